/*
 * cnn_amd.h -- C ABI of libcnn_amd.so: the MI355X (gfx950) replacement for the arithmetic inside
 * hermosayhl/CNN's Layer::forward / Layer::backward / update_gradients (cpu/include/architectures.h:34-138).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 (int32 for the pool mask) unless it says "host";
 *     a batch is contiguous NCHW: sample b of the reference's std::vector<tensor> (data_format.h:53) lives
 *     at base + b*C*H*W, each sample in the reference's own CHW order (data_format.h:11-18);
 *   - weight layouts are the reference's: conv [Co][Ci][k][k] then bias [Co] (conv2d.cpp:18-21,220-226),
 *     linear [in][out] then bias [out] (linear.cpp:40,105-108) -- a .model checkpoint streams straight in;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); every call only ENQUEUES work;
 *   - no allocation inside: scratch comes from the caller (`ws`, sized by the *_workspace_bytes query);
 *   - return value: 0 = ok, non-zero = CNN_AMD_E_* (or 1000 + hipError_t); cnn_amd_last_error() gives text.
 *     The reference has no error channel (assert only), so the host layer classes abort on non-zero.
 */
#ifndef CNN_AMD_H
#define CNN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNN_AMD_ABI_VERSION 2

enum {
    CNN_AMD_OK = 0,
    CNN_AMD_E_BADARG = 1,    /* null pointer / non-positive dimension / unsupported geometry */
    CNN_AMD_E_WORKSPACE = 2, /* ws too small for this call */
    CNN_AMD_E_HIP = 1000,    /* 1000 + hipError_t */
    CNN_AMD_E_COMM = 2000    /* 2000 + ncclResult_t (RCCL); 2000 itself = librccl could not be loaded */
};

int cnn_amd_abi_version(void);
const char* cnn_amd_last_error(void);
/* "gfx950" when a device is present and matches, otherwise an explanatory string; never throws */
const char* cnn_amd_device_arch(void);

/* ---- measurement switches: the A/B switches of DESIGN.md section 10 (kernel-family choices, tile overrides, debug ablations).
 * The library reads the CNN_AMD_* variables of the environment ONCE, when it is first used; afterwards this is the only way to
 * change one (value == NULL removes it).  `name` with or without the "CNN_AMD_" prefix.  Not needed for normal use: the defaults
 * are the product path.  cnn_amd_get_option returns 0 and copies the value when the switch is set, 1 when it is not.
 * CUS=n (n >= 1): every planner sizes its grids, slab counts and tile choices for min(n, the device's compute units) -- a partition
 * of the card, or a test that drives the large-shape branches at a small shape; unset, 0 or negative: the device's own count. */
int cnn_amd_set_option(const char* name, const char* value);
int cnn_amd_get_option(const char* name, char* value_out, size_t cap);
/* Switches that change RESULTS or exist for timing experiments only (a kernel without its stores / DMAs / MFMAs, per-phase cycle
 * printers, an LDS-request override, a data-parallel step without its exchange: DBG, *_DBG, ROWS_LDS, DP_SKIP_EXCHANGE) are compiled
 * out of libcnn_amd.so: cnn_amd_set_option() returns CNN_AMD_E_BADARG for them and the environment is not consulted.  They exist in
 * the measurement build only (make -C cnn_amd/csrc measure -> libcnn_amd_measure.so, loaded by tools/ through CNN_AMD_LIB).
 * cnn_amd_measure_build(): 1 in that build, 0 in the product library. */
int cnn_amd_measure_build(void);

/* ---- measurement: per-kernel durations from HIP events recorded on the launch stream --------------------- */
/* mode 0 = off, 1 = time every kernel launch, 2 = only launches whose "<kernel>|<geometry>" key contains filter */
int cnn_amd_kernel_timing_enable(int mode, const char* filter);
/* mode 2 only: bracket every `every`-th matching launch instead of each one (the two event records around a kernel leave
 * ~6 us bubbles on its stream); the report then counts the sampled launches. */
int cnn_amd_kernel_timing_sampling(int every);
/* device-synchronises; writes "<kernel>|<geometry>\t<launches>\t<total_ms>\n" lines (host buffer) and clears
 * the records; returns bytes needed (records are kept when cap is too small), -1 on error */
long long cnn_amd_kernel_timing_report(char* buf, size_t cap);
/* brackets a span of `stream` that holds NO library kernel -- e.g. the wait for another stream -- with the kernel timer's events: when
 * timing is on it appears in the report under "<name>|span" (give such names the prefix "span:" so that consumers can tell them from
 * kernels); no-ops otherwise.  The host container uses it for "span:exchange_wait": how long the compute stream waits for the
 * gradient exchange at the end of a data-parallel step (the EXPOSED part of the all-reduce). */
int cnn_amd_timing_span_begin(void* stream, const char* name);
int cnn_amd_timing_span_end(void* stream);

/* ---- geometry helpers (host side, pure) -------------------------------------------------------------- */
/* conv2d.cpp:41-42:  out = (H + 2*pad - k)/s + 1, integer division (the reference has pad == 0) */
int cnn_conv2d_out_dim(int in, int k, int s, int pad);
/* pool2d.cpp:14-15:  out = (H - k)/step + 1 */
int cnn_maxpool2d_out_dim(int in, int k, int step);

/* ---- Conv2D : conv2d.cpp --------------------------------------------------------------------------- */
typedef struct {
    int B, Ci, H, W; /* input  batch / channels / height / width */
    int Co, k, s;    /* filters, kernel edge (any k >= 1; the reference asserts odd >= 3), stride */
    int pad;         /* zero padding on each side (extension; the reference is fixed at 0, architectures.h:59) */
    int flags;       /* 0, CNN_CONV2D_POOL_MASK_PACKED (ABI version 2; only the fused Conv2D -> ReLU -> MaxPool2D family reads it) or CNN_CONV2D_DEPTHWISE */
} cnn_conv2d_desc;
/* flags bit: the pool mask the fused first-block entry points (cnn_conv2d_relu_maxpool2_forward*, cnn_conv2d_backward_*pooled2*)
 * write and read is ONE BYTE per window instead of an int32 flat index -- see cnn_conv2d_pool_mask_packed_supported below */
#define CNN_CONV2D_POOL_MASK_PACKED 1
/* flags bit: DEPTHWISE convolution (one filter per channel).  Co == Ci = C, w is [C][1][k][k] (C*k*k floats), bias [C]:
 * y[b][c] = bias[c] + x[b][c] (*) w[c];  gw[c] = (sum_b sum_pq dy * x) / divisor, gb[c] = (sum dy) / divisor;  dx is the gather form
 * (rows / columns no window covers come out +0).  Served by cnn_conv2d_workspace_bytes, cnn_conv2d_forward, _forward_relu,
 * _backward_data, _backward_data_relu, _backward_weight, _backward_weight_side, _backward_workspace_bytes and cnn_conv2d_backward;
 * every other entry that takes a desc refuses the flag (a non-zero status, or 0 from size queries and predicates; the error text
 * says "depthwise").  Both tensors must have fewer than 2^31 elements.  (Value 2 is NOT a flag.) */
#define CNN_CONV2D_DEPTHWISE 4

/* scratch needed by ANY of the three MFMA entry points below for this geometry */
size_t cnn_conv2d_workspace_bytes(const cnn_conv2d_desc* d);

/* Optional, once per geometry and process: times a short list of implicit-GEMM tile shapes for the forward and the data-gradient
 * kernels of this geometry on the device (scratch buffers of its own, zeros; SYNCHRONISES) and pins the fastest for every
 * later call with the same desc -- the built-in rules were tuned on the reference net's layers, other geometries gain up to
 * 2.6x (tools/sweep_igemm.py).  Call it BEFORE cnn_conv2d_prepare_filters / the first forward of the layer (the re-arranged
 * filter image depends on the tile); geometries served by the specialised kernels are left alone.  CNN_AMD_IGEMM_AUTOTUNE=0
 * turns it into a no-op.  The host Conv2D layer calls it when it first sees its input shape. */
int cnn_conv2d_autotune(const cnn_conv2d_desc* d, void* stream);
/* The same measurement with the CALLER's scratch (the header's "no allocation inside" convention; cnn_conv2d_autotune above is the
 * older form that borrows device memory of its own for the duration of the call): scratch of cnn_conv2d_autotune_workspace_bytes(d)
 * bytes (the geometry's input + output + filters + the kernels' workspace).  The host Conv2D layer uses this form. */
size_t cnn_conv2d_autotune_workspace_bytes(const cnn_conv2d_desc* d);
int cnn_conv2d_autotune_ws(const cnn_conv2d_desc* d, void* scratch, size_t scratch_bytes, void* stream);
/* Measured choices are per process; replicas of a data-parallel job should run the SAME kernels (their reduced gradients are identical
 * either way, their local activations then are too).  export: what this process pinned for the geometry, four integers --
 * [0] forward tile, [1] data-gradient tile (-1 = the rule-based default measured best), [2] / [3] = 1 when the implicit GEMM replaces
 * the register-direct forward / data-gradient kernel; CNN_TUNE_NONE = never measured.  import: pins them in another process (entries
 * equal to CNN_TUNE_NONE leave its table alone).  Ship them with cnn_comm_broadcast; the host container does (Sequential::set_comm). */
#define CNN_TUNE_NONE (-2147483647 - 1)
int cnn_conv2d_tune_export(const cnn_conv2d_desc* d, int32_t out[4]);
int cnn_conv2d_tune_import(const cnn_conv2d_desc* d, const int32_t in[4]);

/* replaces Conv2D::forward's loop nest (conv2d.cpp:69-92): y = bias + valid cross-correlation.
 * Implicit GEMM on v_mfma_f32_32x32x2_f32 / 16x16x4_f32, input rows + filter slabs staged in LDS. */
int cnn_conv2d_forward(const cnn_conv2d_desc* d, const float* x, const float* w, const float* bias, float* y,
                       void* ws, size_t ws_bytes, void* stream);
/* Conv2D::forward immediately followed by ReLU::forward (relu.cpp:21-26) in ONE kernel: y as above AND
 * y_relu = (y >= 0 ? y : 0), both NCHW tensors are written (the convolution output stays observable, alexnet.cpp:97);
 * saves the ReLU kernel's re-read of y.  Bit-identical to cnn_conv2d_forward + cnn_relu_forward. */
int cnn_conv2d_forward_relu(const cnn_conv2d_desc* d, const float* x, const float* w, const float* bias, float* y,
                            float* y_relu, void* workspace, size_t workspace_bytes, void* stream);
/* != 0: cnn_conv2d_forward_relu / cnn_conv2d_forward_prepared accept y == NULL for this layer and then write ONLY y_relu
 * (a training step never reads the pre-activation tensor: ReLU::backward masks by its own output, relu.cpp:35-40). */
int cnn_conv2d_relu_only_supported(const cnn_conv2d_desc* d);

/* The reference's first block Conv2D -> ReLU -> MaxPool2D(2, 2) (alexnet.cpp:12-15; conv2d.cpp:69-92, relu.cpp:21-26,
 * pool2d.cpp:53-87) in ONE kernel: pooled [B][Co][Ho/2][Wo/2] and mask (same meaning as cnn_maxpool2d_forward: flat index
 * into the sample's Co*Ho*Wo of the window's first maximum; may be NULL) are bit-identical to cnn_conv2d_forward_relu +
 * cnn_maxpool2d_forward, but the convolution / ReLU outputs are NOT materialised -- nothing downstream needs them: the
 * backward pass takes pooled + mask (cnn_maxpool2d_backward_relu, cnn_conv2d_backward_*_pooled2).
 * Bit 31 of a mask entry is additionally SET when that window's pooled value is <= 0, i.e. when the block's ReLU::backward
 * (relu.cpp:37) blocks the window's delta: the pooled-domain gradient entry points below compare the entry with the flat index they
 * expect and therefore skip such windows by themselves (pass pooled = NULL: no tensor is read for the ReLU mask anywhere in the
 * backward pass); cnn_maxpool2d_backward(_relu) ignore the bit.  (mask & 0x7fffffff) is cnn_maxpool2d_forward's mask, bit for bit.
 * Covered geometry: cnn_conv2d_relu_maxpool2_supported(d) != 0 (the thin 3 -> 16 channel 3x3 stride-2 layer). */
int cnn_conv2d_relu_maxpool2_supported(const cnn_conv2d_desc* d);
/* The packed pool mask (d->flags & CNN_CONV2D_POOL_MASK_PACKED).  A 2x2 window's first maximum is one of FOUR pixels, so the int32
 * flat index carries two bits of information in four bytes -- and the three kernels of the block (forward, weight gradient, data
 * gradient) move it through HBM once each: 3 x 49.6 MB per step of the reference net at batch 256.  With the flag set the mask
 * argument of the family is an opaque buffer of cnn_conv2d_pool_mask_bytes(d) bytes (device, 4-byte aligned) holding
 *   byte[((b * Co + co) * (Ho/2) + ph) * pitch + pw],  pitch = ((Wo/2) + 3) & ~3,
 *   bits 0..1 = 2 * (row of the maximum inside the window) + (its column), bit 7 = the int32 form's bit 31 (pooled value <= 0),
 * written by cnn_conv2d_relu_maxpool2_forward(_prepared) and read by the cnn_conv2d_backward_*pooled2* calls with the SAME desc
 * (pooled must then be NULL: bit 7 carries the block's ReLU mask).  cnn_conv2d_pool_mask_unpack converts it to the int32 form
 * (bit 31 included) for anybody else -- cnn_maxpool2d_backward(_relu) read only that one.  Results of every call of the family are
 * bit-identical between the two forms.  supported(d) != 0: the geometry is covered AND the kernels that read the packed form are
 * the ones selected (measurement switches that select the older kernels turn it off); a call with the flag set otherwise fails
 * with CNN_AMD_E_BADARG. */
int cnn_conv2d_pool_mask_packed_supported(const cnn_conv2d_desc* d);
size_t cnn_conv2d_pool_mask_bytes(const cnn_conv2d_desc* d); /* flag clear: B*Co*(Ho/2)*(Wo/2)*4; set: B*Co*(Ho/2)*pitch + 64 */
int cnn_conv2d_pool_mask_unpack(const cnn_conv2d_desc* d, const void* packed, int32_t* mask, void* stream);
int cnn_conv2d_relu_maxpool2_forward(const cnn_conv2d_desc* d, const float* x, const float* w, const float* bias,
                                     float* pooled, int32_t* mask, void* workspace, size_t workspace_bytes, void* stream);

/* Conv2D::backward of that block when the delta of the convolution output exists only in the pooled domain:
 *   dy = ReLU::backward(MaxPool2D::backward(dpool))   (relu.cpp:35-40, pool2d.cpp:96-107)
 * is rebuilt on the fly from dpool (delta of the pool output), mask and pooled (both as written by the forward call), so
 * the Co*Ho*Wo delta tensor is never written or read.  Results are bit-identical to cnn_maxpool2d_backward_relu followed by
 * cnn_conv2d_backward_weight / cnn_conv2d_backward_data.  pooled == NULL: dpool already carries the ReLU mask
 * ((pooled <= 0) ? 0 : dpool, e.g. from cnn_conv2d_backward_data_relu(..., relu_below = pooled, ...) of the next layer). */
int cnn_conv2d_backward_weight_pooled2(const cnn_conv2d_desc* d, const float* x, const float* dpool, const int32_t* mask,
                                       const float* pooled, float* gw, float* gb, float divisor, void* workspace,
                                       size_t workspace_bytes, void* stream);
int cnn_conv2d_backward_data_pooled2(const cnn_conv2d_desc* d, const float* dpool, const int32_t* mask, const float* pooled,
                                     const float* w, float* dx, void* workspace, size_t workspace_bytes, void* stream);
/* cnn_conv2d_backward_weight_pooled2 followed -- in ONE more launch instead of three -- by this layer's share of the end of a
 * single-rank train step: gw/gb as above, then w/bias -= lr * (grad_scale * gw/gb) (cnn_sgd_update's arithmetic, alexnet.cpp:62-65
 * -> conv2d.cpp update_gradients) and the layer's prepared filters (cnn_conv2d_prepare_filters images of the UPDATED w/bias;
 * either may be NULL).  Bit-identical to the three separate calls.  workspace as for cnn_conv2d_backward_weight_pooled2. */
int cnn_conv2d_backward_weight_pooled2_sgd(const cnn_conv2d_desc* d, const float* x, const float* dpool, const int32_t* mask,
                                           const float* pooled, float* gw, float* gb, float divisor, float* w, float* bias, float lr,
                                           float grad_scale, void* fwd_prepared, void* dgrad_prepared, void* workspace,
                                           size_t workspace_bytes, void* stream);

/* ... and additionally stores the filters / biases as they were BEFORE the step into w_previous [Co][Ci*k*k] / bias_previous [Co]
 * (either may be NULL).  The host container keeps that snapshot so that Layer::get_output() of a layer whose output tensor was fused
 * away can still be re-computed with the parameters the last forward pass used (alexnet.cpp:97,105), after the step has moved them. */
int cnn_conv2d_backward_weight_pooled2_sgd_keep(const cnn_conv2d_desc* d, const float* x, const float* dpool, const int32_t* mask,
                                                const float* pooled, float* gw, float* gb, float divisor, float* w, float* bias, float lr,
                                                float grad_scale, void* fwd_prepared, void* dgrad_prepared, float* w_previous,
                                                float* bias_previous, void* workspace, size_t workspace_bytes, void* stream);

/* replaces conv2d.cpp:117-159: gw = (sum_b sum_pq dy*x)/divisor, gb = (sum_b sum_pq dy)/divisor.
 * The reference divides by the batch size per sample and accumulates (:148,:157); pass divisor = B of the
 * WHOLE batch (per-rank shard size under data parallelism, see cnn_sgd_update).  gb may be NULL.
 * Split-K over pixels with a deterministic second-stage reduction (no atomics). */
int cnn_conv2d_backward_weight(const cnn_conv2d_desc* d, const float* x, const float* dy, float* gw, float* gb,
                               float divisor, void* ws, size_t ws_bytes, void* stream);

/* replaces conv2d.cpp:168-199 (zero fill + scatter-add) by the equivalent gather: transposed implicit GEMM,
 * stride handled by output-parity classes; input rows/cols no window covers come out 0 like the reference. */
int cnn_conv2d_backward_data(const cnn_conv2d_desc* d, const float* dy, const float* w, float* dx, void* ws,
                             size_t ws_bytes, void* stream);
/* Conv2D data gradient followed by the ReLU::backward (relu.cpp:35-40) of the ReLU layer in front of this convolution:
 * relu_below = that layer's forward output (same shape as dx); dx = (relu_below <= 0 ? 0 : dx), applied in the kernel's
 * store epilogue.  Bit-identical to cnn_conv2d_backward_data + cnn_relu_backward(relu_below, dx). */
int cnn_conv2d_backward_data_relu(const cnn_conv2d_desc* d, const float* dy, const float* w, const float* relu_below,
                                  float* dx, void* workspace, size_t workspace_bytes, void* stream);

/* Conv2D::backward (conv2d.cpp:97-202) in one call: the weight/bias-gradient kernels run on an internal side stream
 * CONCURRENTLY with the data-gradient kernels (fork/join by events on `stream`; hipGraph-capturable).  Same results as
 * the two separate calls.  gb may be NULL. */
size_t cnn_conv2d_backward_workspace_bytes(const cnn_conv2d_desc* d);
/* defer_join = 0: gw/gb/dx are all ordered on `stream` when the call returns.  defer_join = 1: only dx is; gw/gb (and this
 * call's half of ws) belong to the side stream until cnn_amd_side_stream_join(stream) -- lets the weight gradients of
 * layer L overlap the whole backward of layers L-1.. (the caller joins once, before it reads the gradient arena).  With
 * defer_join = 1 the final reduction of the layer's partial gradient slabs (held in ws) is only recorded; the join launches
 * the recorded reductions of the calling thread in one batch (join from the thread that made the calls): ws must not be
 * reused, and gw/gb are undefined, until then. */
int cnn_conv2d_backward(const cnn_conv2d_desc* d, const float* x, const float* dy, const float* w, float* gw, float* gb,
                        float* dx, float divisor, void* ws, size_t ws_bytes, void* stream, int defer_join);
/* Scope of the hidden state behind defer_join (VERDICT r03 asked): the side stream, its fork / join events and the list of recorded
 * slab reductions exist once per (host thread, device), NOT per caller stream.  A thread that forks weight gradients off two different
 * streams of one device gets them serialised on the one side stream; cnn_amd_side_stream_join(S) launches EVERY recorded reduction of the
 * thread (also those forked off another stream) and makes S wait for the side stream as a whole -- conservative, never too weak: a later
 * join from the other stream finds nothing left to launch and waits for the same work.  Two host threads never share any of it. */
int cnn_amd_side_stream_join(void* stream);
/* The weight / bias-gradient half of cnn_conv2d_backward(defer_join = 1) alone: the kernels run on the side stream, forked off `stream`
 * where the call is made (x and dy must be ordered on `stream` by then); gw / gb / ws belong to the side stream until
 * cnn_amd_side_stream_join(stream).  For callers that obtain the data gradients of several layers another way
 * (e.g. one fused kernel of their own).  workspace: cnn_conv2d_workspace_bytes(d). */
int cnn_conv2d_backward_weight_side(const cnn_conv2d_desc* d, const float* x, const float* dy, float* gw, float* gb, float divisor,
                                    void* workspace, size_t workspace_bytes, void* stream);
/* For callers that schedule more work behind the deferred weight gradients (e.g. the SGD step and the re-prepared filters of the
 * layers whose gradients are complete, while the first layers' backward kernels still run on `stream`):
 *   cnn_amd_side_stream_get   the side stream (hipStream_t) of the calling thread on the current device;
 *   cnn_amd_flush_reduces     launches the recorded slab reductions of the calling thread on `stream` NOW -- normally the side
 *                             stream -- instead of at the join (gw/gb of those layers are then ordered on that stream). */
int cnn_amd_side_stream_get(void** side_stream);
int cnn_amd_flush_reduces(void* stream);
/* Cross-stream dependencies without a marker packet on the producing stream (an event recorded BETWEEN two kernels costs that
 * stream ~4.5 us on this hardware; an event carried by the producing kernel's own dispatch ~1.7 us):
 *   cnn_amd_publish_next_kernel(stream)  the next kernel this thread launches on `stream` through the library publishes its
 *                                        completion (forward, data-gradient and linear-backward kernels of the reference net
 *                                        carry it in their dispatch packet; any other kernel is followed by a plain event record);
 *   cnn_amd_wait_published(other)        `other` waits for that kernel = cnn_event_record + cnn_stream_wait_event.
 * cnn_conv2d_backward*() use the published kernel as their fork point when it is the last thing the library launched on
 * `stream`: the caller asserts that nothing else the weight gradient depends on was queued on that stream behind it. */
int cnn_amd_publish_next_kernel(void* stream);
int cnn_amd_wait_published(void* stream);
/* != 0: a published kernel exists on `stream` and it is the LAST thing this thread queued on that stream through the library
 * (kernels, copies, waits, collectives) -- i.e. cnn_amd_wait_published(other) is equivalent to record + wait right now. */
int cnn_amd_published_is_last(void* stream);

/* im2col + plain tiled GEMM: functional fallback kept ONLY for parity checks of the three calls above */
size_t cnn_conv2d_im2col_workspace_bytes(const cnn_conv2d_desc* d);
int cnn_conv2d_forward_im2col(const cnn_conv2d_desc* d, const float* x, const float* w, const float* bias,
                              float* y, void* ws, size_t ws_bytes, void* stream);
int cnn_conv2d_backward_weight_im2col(const cnn_conv2d_desc* d, const float* x, const float* dy, float* gw,
                                      float* gb, float divisor, void* ws, size_t ws_bytes, void* stream);
int cnn_conv2d_backward_data_im2col(const cnn_conv2d_desc* d, const float* dy, const float* w, float* dx,
                                    void* ws, size_t ws_bytes, void* stream);

/* ---- MaxPool2D : pool2d.cpp ------------------------------------------------------------------------ */
/* replaces pool2d.cpp:53-87. mask (may be NULL = the no_grad path, :41,:61,:79) receives the int32 flat index
 * into the sample's C*H*W of each window's FIRST maximum (strict '<', :71).  Bit-exact vs the reference. */
int cnn_maxpool2d_forward(const float* x, float* y, int32_t* mask, int B, int C, int H, int W, int k, int step,
                          void* stream);
/* replaces pool2d.cpp:96-107: dx = 0; dx[mask[i]] = dy[i] (assignment; with overlapping windows the highest
 * output index wins, reproduced deterministically). */
int cnn_maxpool2d_backward(const float* dy, const int32_t* mask, float* dx, int B, int C, int H, int W, int k,
                           int step, void* stream);
/* MaxPool2D::backward immediately followed by the ReLU::backward (relu.cpp:35-40) of the ReLU layer whose output was
 * this pool's input, in ONE kernel.  pooled = the pool's forward output y: at an argmax position the ReLU output equals
 * pooled[window], everywhere else the delta is 0 either way, so dx[argmax] = (pooled <= 0 ? 0 : dy) reproduces
 * cnn_maxpool2d_backward + cnn_relu_backward bit for bit without reading the ReLU output tensor. */
int cnn_maxpool2d_backward_relu(const float* dy, const int32_t* mask, const float* pooled, float* dx, int B, int C, int H,
                                int W, int k, int step, void* stream);

/* ---- ReLU : relu.cpp ------------------------------------------------------------------------------- */
/* relu.cpp:21-26: y = x >= 0 ? x : 0   (keeps -0.0, NaN -> 0) */
int cnn_relu_forward(const float* x, float* y, size_t n, void* stream);
/* relu.cpp:35-40: dy = (y <= 0) ? 0 : dy, IN PLACE on the caller's delta */
int cnn_relu_backward(const float* y, float* dy_inout, size_t n, void* stream);

/* ---- Dropout : dropout.cpp (row n4 of SURVEY.md 8f; the reference keeps it out of its net, alexnet.cpp:28) -------------
 * Channel dropout as the reference implements it: training (dropout.cpp:34-41) zeroes channels 0 .. dropped_channels-1 of every
 * sample (dropped_channels = int(p * C), :18; the shuffled sequence never reaches the data path) and copies the rest; under
 * no_grad (:44-53) y = x * keep with keep = 1 - p.  backward (:57-69) zeroes the same channels of the delta IN PLACE. */
int cnn_dropout_forward(const float* x, float* y, int B, int C, int H, int W, int dropped_channels, int training, float keep,
                        void* stream);
int cnn_dropout_backward(float* dy_inout, int B, int C, int H, int W, int dropped_channels, void* stream);

/* ---- LinearLayer : linear.cpp ---------------------------------------------------------------------- */
/* linear.cpp:33-43: y[b][j] = (sum_i x[b][i]*W[i*out+j]) + bias[j] */
int cnn_linear_forward(const float* x, const float* w, const float* bias, float* y, int B, int in, int out,
                       void* stream);
/* linear.cpp:56-90: gW = (x^T dy)/divisor (assigned), gb = (sum_b dy)/divisor, dx = dy W^T; any output may be NULL */
int cnn_linear_backward(const float* x, const float* dy, const float* w, float* gw, float* gb, float* dx, int B,
                        int in, int out, float divisor, void* stream);
/* Linear::backward followed by the ReLU::backward (relu.cpp:35-40) of the ReLU layer whose OUTPUT is this layer's input x:
 * dx = (x <= 0 ? 0 : dx).  Bit-identical to cnn_linear_backward + cnn_relu_backward(x, dx). */
int cnn_linear_backward_relu(const float* x, const float* dy, const float* w, float* gw, float* gb, float* dx, int B,
                             int in, int out, float divisor, void* stream);

/* ---- optional: filter preparation hoisted out of the per-layer calls ----------------------------------
 * cnn_conv2d_forward / cnn_conv2d_backward_data re-arrange the filters for their kernels in a small launch of their own
 * on every call, because the filters may have changed (Conv2D::update_gradients, conv2d.cpp:205-217).  A caller that
 * knows WHEN they change -- once per SGD step -- can re-arrange the filters of all layers with one or two launches and
 * pass the results in; outputs are bit-identical to the plain calls.
 *   fwd[i] / dgrad[i]: device buffers of cnn_conv2d_prepared_bytes(&descs[i]) bytes each (NULL entries / arrays skip that
 *   mode); they must be re-prepared after every change of w[i] / bias[i].  At most 6 layers per call. */
size_t cnn_conv2d_prepared_bytes(const cnn_conv2d_desc* d);
int cnn_conv2d_prepare_filters(int n, const cnn_conv2d_desc* descs, const float* const* w, const float* const* bias,
                               void* const* fwd, void* const* dgrad, void* stream);
/* cnn_conv2d_forward / _forward_relu (y_relu nullable) from prepared filters */
int cnn_conv2d_forward_prepared(const cnn_conv2d_desc* d, const float* x, const void* prepared_fwd, const float* bias,
                                float* y, float* y_relu, void* stream);
int cnn_conv2d_backward_data_prepared(const cnn_conv2d_desc* d, const float* dy, const void* prepared_dgrad, float* dx,
                                      void* stream);
/* cnn_conv2d_relu_maxpool2_forward from prepared filters (the bias is part of the prepared buffer) */
int cnn_conv2d_relu_maxpool2_forward_prepared(const cnn_conv2d_desc* d, const float* x, const void* prepared_fwd,
                                              float* pooled, int32_t* mask, void* stream);
int cnn_conv2d_backward_data_pooled2_prepared(const cnn_conv2d_desc* d, const float* dpool, const int32_t* mask,
                                              const float* pooled, const void* prepared_dgrad, float* dx, void* stream);
int cnn_conv2d_backward_data_relu_prepared(const cnn_conv2d_desc* d, const float* dy, const void* prepared_dgrad,
                                           const float* relu_below, float* dx, void* stream);
/* cnn_conv2d_backward_weight_pooled2 (side stream) + cnn_conv2d_backward_data_pooled2_prepared in one call, like
 * cnn_conv2d_backward_prepared */
int cnn_conv2d_backward_pooled2_prepared(const cnn_conv2d_desc* d, const float* x, const float* dpool, const int32_t* mask,
                                         const float* pooled, const void* prepared_dgrad, float* gw, float* gb, float* dx,
                                         float divisor, void* workspace, size_t workspace_bytes, void* stream, int defer_join);
/* cnn_conv2d_backward with the data gradient from prepared filters; workspace: cnn_conv2d_workspace_bytes(d) */
int cnn_conv2d_backward_prepared(const cnn_conv2d_desc* d, const float* x, const float* dy, const void* prepared_dgrad,
                                 float* gw, float* gb, float* dx, float divisor, void* workspace, size_t workspace_bytes,
                                 void* stream, int defer_join);
/* ... and with the ReLU::backward of the layer in front fused into the data gradient (relu_below nullable) */
int cnn_conv2d_backward_prepared_relu(const cnn_conv2d_desc* d, const float* x, const float* dy, const void* prepared_dgrad,
                                      const float* relu_below, float* gw, float* gb, float* dx, float divisor,
                                      void* workspace, size_t workspace_bytes, void* stream, int defer_join);

/* ---- BatchNorm2D : batchnorm2d.cpp:24-95 (forward), :98-158 (backward) ------------------------------- */
/* Per-channel statistics over (B,H,W) of an NCHW tensor; gamma/beta/moving_mean/moving_var/saved_* are [C].
 * training != 0 (the reference's !no_grad branch, :46-80): two-pass batch mean and BIASED variance are written to
 *   saved_mean / saved_var (the reference's buffer_mean / buffer_var), y = gamma*((x-mean)/sqrt(var+eps)) + beta, and
 *   moving = (1-momentum)*moving + momentum*stat (moving statistics start at 0/0 in the reference, :20).
 * training == 0 (:82-93): the moving statistics are used; saved_* / workspace may be NULL.
 * The reference's normed_input buffer is not produced: backward recomputes it from x and saved_*.
 * x / y / dy must be 16-byte aligned.  workspace: cnn_batchnorm2d_workspace_bytes(B,C,H,W) bytes. */
size_t cnn_batchnorm2d_workspace_bytes(int B, int C, int H, int W);
int cnn_batchnorm2d_forward(const float* x, float* y, const float* gamma, const float* beta, float* moving_mean,
                            float* moving_var, float* saved_mean, float* saved_var, int B, int C, int H, int W,
                            float eps, float momentum, int training, void* workspace, size_t workspace_bytes,
                            void* stream);
/* BatchNorm2D followed by a ReLU layer (every BN site of the ResNet-shaped stack): y as above AND y_relu = relu(y)
 * (relu.cpp:25) from the same pass -- the ReLU layer's own kernel would read y again.  y_relu: 16-byte aligned, same shape as y.
 * y may be NULL (round 4): then only y_relu is written -- a train step never reads the normalised tensor itself (ReLU::backward masks by
 * its own output, BatchNorm2D::backward recomputes from x and saved_*); cnn_batchnorm2d_forward(training = 0) with saved_mean / saved_var
 * in the place of the moving statistics re-computes y bit for bit when somebody asks for it (the host layer's get_output() does). */
int cnn_batchnorm2d_forward_relu(const float* x, float* y, float* y_relu, const float* gamma, const float* beta,
                                 float* moving_mean, float* moving_var, float* saved_mean, float* saved_var, int B, int C, int H,
                                 int W, float eps, float momentum, int training, void* workspace, size_t workspace_bytes,
                                 void* stream);
/* BatchNorm2D -> ReLU -> MaxPool2D(2, 2) (round 6): the apply pass also pools -- pooled [B][C][H/2][W/2] and pool_mask (int32 flat index into
 * the sample, pool2d.cpp:81; NULL: not recorded) are what cnn_maxpool2d_forward would make of y_relu, bit for bit (the pool's scan order and
 * strict '<').  y and y_relu are each written only when non-NULL: a train step needs neither (cnn_batchnorm2d_backward_pooled takes the
 * ReLU's test from `pooled`).  H, W even, channels beyond the one-workgroup limit (_supported answers 1); tensors 8-byte aligned. */
int cnn_batchnorm2d_forward_relu_pool_supported(int B, int C, int H, int W);
int cnn_batchnorm2d_forward_relu_pool(const float* x, float* y, float* y_relu, float* pooled, int32_t* pool_mask, const float* gamma,
                                      const float* beta, float* moving_mean, float* moving_var, float* saved_mean, float* saved_var, int B,
                                      int C, int H, int W, float eps, float momentum, int training, void* workspace, size_t workspace_bytes,
                                      void* stream);
/* dy is overwritten with dx IN PLACE, like the reference (:149-155).  ggamma[c] = sum dy*norm, gbeta[c] = sum dy:
 * plain sums over (B,H,W), NOT divided by the batch (:123-124).  x is the forward input, saved_* the batch
 * statistics of that forward call. */
int cnn_batchnorm2d_backward(const float* x, float* dy, const float* gamma, const float* saved_mean,
                             const float* saved_var, float* ggamma, float* gbeta, int B, int C, int H, int W, float eps,
                             void* workspace, size_t workspace_bytes, void* stream);
/* BatchNorm2D <- ReLU <- MaxPool2D(2, 2) (round 6): cnn_maxpool2d_backward_relu + cnn_batchnorm2d_backward without the tensor in between.
 * The delta at the normalisation's output is REBUILT from the pooled domain -- dpool [B][C][H/2][W/2] (the pool's incoming delta), mask (the
 * pool's int32 flat index into the sample, pool2d.cpp:81) and pooled (the pool's output = the ReLU output at the maximum: relu.cpp:37's test)
 * -- inside the two backward kernels, which walk the same elements in the same order with the same arithmetic as cnn_batchnorm2d_backward:
 * ggamma, gbeta and dx are BIT-IDENTICAL to the three-call sequence.  dx [B][C][H][W] is written (nothing is read there).  H even, W a
 * multiple of 4 (_supported answers 1); x / dx 16-byte, dpool / mask / pooled 8-byte aligned; workspace as cnn_batchnorm2d_backward's. */
int cnn_batchnorm2d_backward_pooled_supported(int B, int C, int H, int W);
int cnn_batchnorm2d_backward_pooled(const float* x, const float* dpool, const int32_t* mask, const float* pooled, float* dx,
                                    const float* gamma, const float* saved_mean, const float* saved_var, float* ggamma, float* gbeta,
                                    int B, int C, int H, int W, float eps, void* workspace, size_t workspace_bytes, void* stream);

/* BatchNorm2D with the batch SHARDED over data-parallel processes ("sync-BN"): the reference normalises over the whole
 * batch (batchnorm2d.cpp:46-63), so each rank computes per-channel partial sums, the caller all-reduces (sum) the small
 * vectors between the calls, and the apply kernels use the GLOBAL element count `count` = B_global*H*W.  Training step:
 *   cnn_batchnorm2d_partial_sums(x, NULL, 0, s1)              all-reduce s1[C]     (sum of x)
 *   cnn_batchnorm2d_partial_sums(x, s1, count, s2)            all-reduce s2[C]     (sum of (x - s1/count)^2: two-pass)
 *   cnn_batchnorm2d_forward_from_sums(..., s1, s2, count)     mean / biased variance -> saved_*, moving_*, y
 *   cnn_batchnorm2d_backward_sums(x, dy, ..., sums4)          all-reduce sums4[C][4]
 *   cnn_batchnorm2d_backward_from_sums(..., sums4, count)     dy -> dx in place; ggamma / gbeta = the FULL-batch sums
 *                                                             (identical on every rank: exclude them from the gradient
 *                                                             all-reduce or divide by the world size afterwards)
 * With one process this is the arithmetic of cnn_batchnorm2d_forward / _backward on their general path (layers whose channels
 * fit LDS take a one-workgroup-per-channel kernel there, which sums a channel in a different order: equal within rounding).
 * Evaluation needs no exchange. */
int cnn_batchnorm2d_partial_sums(const float* x, const float* sum_x, float count, float* out, int B, int C, int H, int W,
                                 void* workspace, size_t workspace_bytes, void* stream);
int cnn_batchnorm2d_forward_from_sums(const float* x, float* y, const float* gamma, const float* beta, float* moving_mean,
                                      float* moving_var, float* saved_mean, float* saved_var, const float* sum_x,
                                      const float* sum_sq, float count, int B, int C, int H, int W, float eps,
                                      float momentum, void* stream);
/* ... with the ReLU output of the layer behind it from the same pass (see cnn_batchnorm2d_forward_relu) */
int cnn_batchnorm2d_forward_from_sums_relu(const float* x, float* y, float* y_relu, const float* gamma, const float* beta,
                                           float* moving_mean, float* moving_var, float* saved_mean, float* saved_var,
                                           const float* sum_x, const float* sum_sq, float count, int B, int C, int H, int W,
                                           float eps, float momentum, void* stream);
int cnn_batchnorm2d_backward_sums(const float* x, const float* dy, const float* gamma, const float* saved_mean,
                                  const float* saved_var, float* sums4, int B, int C, int H, int W, float eps,
                                  void* workspace, size_t workspace_bytes, void* stream);
int cnn_batchnorm2d_backward_from_sums(const float* x, float* dy, const float* gamma, const float* saved_mean,
                                       const float* saved_var, const float* sums4, float count, float* ggamma,
                                       float* gbeta, int B, int C, int H, int W, float eps, void* stream);

/* ---- SGD step : conv2d.cpp:205-217, linear.cpp:95-102 ---------------------------------------------- */
/* p -= lr * (g * grad_scale) over one flat parameter arena.  grad_scale = 1 reproduces the reference exactly
 * (two roundings, no FMA); grad_scale = 1/G folds the data-parallel mean after an all-reduce(sum) over G ranks
 * whose kernels each divided by their local batch. */
int cnn_sgd_update(float* params, const float* grads, size_t n, float lr, float grad_scale, void* stream);
/* the same step; previous[i] (nullable) receives params[i] as it was before (see cnn_conv2d_backward_weight_pooled2_sgd_keep) */
int cnn_sgd_update_keep(float* params, const float* grads, size_t n, float lr, float grad_scale, float* previous, void* stream);

/* SGD with momentum, weight decay and Nesterov over a range of the flat arena -- the update of torch.optim.SGD with dampening 0,
 * in cnn_sgd_update's arithmetic (fp32, every product and sum rounded separately, no FMA).  Per element i:
 *     gs = grad_scale != 1 ? g * grad_scale : g
 *     d  = (decays(i) && weight_decay != 0) ? gs + weight_decay * p : gs
 *     momentum == 0 :  u = d                                     (velocity is neither read nor written, and may be NULL)
 *     otherwise     :  v' = momentum * v + d ;  u = nesterov ? d + momentum * v' : v'
 *     p' = p - lr * u
 * velocity: n floats of state, zero before the first step.  previous (nullable) as in cnn_sgd_update_keep.  With momentum == 0 and
 * weight_decay == 0 the result equals cnn_sgd_update_keep's bit for bit.
 * decays(i): weight decay applies inside n_ranges half-open index ranges only -- a layer's weights, not BatchNorm2D's moving
 * statistics, which share the arena.  decay_ranges is a HOST array of 2 * n_ranges values, begin then end of every range, relative
 * to the `params` pointer of this call, ascending, non-empty and disjoint, end <= n (checked).  Up to CNN_SGD_INLINE_RANGES ranges
 * travel in the kernel arguments; beyond that the kernel reads them from decay_ranges_dev, a DEVICE copy of the same array that
 * the caller keeps (NULL is fine for smaller tables).  n <= 2^32 - 257 per call (the table is 32-bit).
 * One call is one kernel launch, whatever the number of ranges: 20 bytes per element, 24 with `previous`. */
typedef struct cnn_sgd_options {
    float lr;
    float momentum;     /* >= 0 */
    float weight_decay; /* >= 0 */
    int nesterov;       /* 0 / 1 */
} cnn_sgd_options;
#define CNN_SGD_INLINE_RANGES 64
int cnn_sgd_momentum_update(float* params, const float* grads, float* velocity, size_t n, const cnn_sgd_options* opt, float grad_scale,
                            const uint32_t* decay_ranges, const uint32_t* decay_ranges_dev, size_t n_ranges, float* previous,
                            void* stream);

/* Adam / AdamW over a range of the flat arena -- the update of torch.optim.Adam / AdamW with amsgrad off, in
 * cnn_sgd_momentum_update's arithmetic: fp32, every product, sum, quotient and root rounded separately (no FMA), the quotient and the
 * root correctly rounded, denormals kept.  Host scalars of the call:
 *     om   = 1.f - lr * weight_decay   (two fp32 operations)       omb1 = 1.f - beta1, omb2 = 1.f - beta2   (fp32)
 *     bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step))   ss   = (float)((double)lr / (1.0 - pow((double)beta1, (double)step)))
 * Per element i:
 *     gs  = grad_scale != 1 ? g * grad_scale : g
 *     dec = decays(i) && weight_decay != 0
 *     d   = (dec && !decoupled) ? gs + weight_decay * p : gs
 *     p0  = (dec &&  decoupled) ? p * om : p
 *     m'  = beta1 * m + omb1 * d
 *     v'  = beta2 * v + omb2 * (d * d)
 *     den = sqrt(v') / bc2s + eps
 *     q   = m' / den
 *     p'  = p0 - ss * q
 * exp_avg (m), exp_avg_sq (v): n floats of state each, zero before the first step.  grad_scale, previous, decays(i), decay_ranges,
 * decay_ranges_dev, n_ranges and the limit on n are cnn_sgd_momentum_update's.  Checked before any launch: beta1, beta2 in [0, 1),
 * eps > 0, weight_decay >= 0, step >= 1, the range table.  One call is one kernel launch: 28 bytes per element, 32 with `previous`. */
typedef struct cnn_adam_options {
    float lr, beta1, beta2, eps, weight_decay;
    int decoupled;        /* 0: Adam (L2 term added to the gradient)   1: AdamW (parameter shrunk by 1 - lr * wd) */
    uint64_t step;        /* 1-based number of THIS step */
} cnn_adam_options;
int cnn_adam_update(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, const cnn_adam_options* opt,
                    float grad_scale, const uint32_t* decay_ranges, const uint32_t* decay_ranges_dev, size_t n_ranges,
                    float* previous, void* stream);

/* Clipping by the global L2 norm of one flat gradient range -- torch.nn.utils.clip_grad_norm_ (error_if_nonfinite=False) without a
 * host round trip:
 *     S      = sum_i (double)g[i] * (double)g[i]                (fp64: per-workgroup partials in `workspace`, summed in a fixed order,
 *                                                                no floating-point atomics -- the same words from run to run)
 *     norm   = (float)sqrt(S)
 *     total  = grad_scale != 1 ? norm * grad_scale : norm       (fp32)
 *     c      = max_norm / (total + 1e-6f)                       (fp32, two operations)
 *     coef   = c < 1 ? c : 1                                    (a NaN total leaves coef = 1)
 *     g[i]   = g[i] * coef                                      only when coef < 1; otherwise the range is not written
 *     stats_dev[0] = total, stats_dev[1] = coef                 (device memory, two floats)
 * workspace: device memory, 8-byte aligned, at least cnn_clip_grad_norm_workspace_bytes(n) bytes (never more than
 * 8 * CNN_CLIP_MAX_BLOCKS).  max_norm > 0, n > 0 (checked).  Three kernel launches per call, the host never waits. */
#define CNN_CLIP_MAX_BLOCKS 2048
size_t cnn_clip_grad_norm_workspace_bytes(size_t n);
int cnn_clip_grad_norm(float* grads, size_t n, float max_norm, float grad_scale, void* workspace, size_t workspace_bytes,
                       float* stats_dev /* [2]: total norm, coefficient */, void* stream);

/* Gradient accumulation over micro-batches: one streaming pass that folds the gradients of one backward pass into an accumulator.
 *     first != 0 :  acc[i] = grads[i]             a copy of the bits -- -0.0, infinities, NaN payloads and denormals come out as they
 *                                                 went in; acc is not read (it may hold anything), 8 bytes per element
 *     first == 0 :  acc[i] = acc[i] + grads[i]    one fp32 add, denormals kept, 12 bytes per element
 * A window of k passes is one call with first = 1 and k - 1 with first = 0: acc = ((g1 + g2) + g3) + ..., the order a host loop
 * would use.  acc and grads may be misaligned independently (a pointer that is not 16-byte aligned takes the scalar kernel).  Checked
 * before any launch: no null pointer, n > 0, acc != grads.  One kernel launch per call (its name begins with gacc_). */
int cnn_grad_accumulate(float* acc, const float* grads, size_t n, int first, void* stream);

/* Exponential moving average of the parameters (torch.optim.swa_utils.AveragedModel, timm's ModelEmaV2, TF's
 * ExponentialMovingAverage): one streaming pass that folds the current parameters into a shadow copy of the arena, in
 * cnn_sgd_momentum_update's arithmetic (fp32, every product and sum rounded separately, no FMA, denormals kept).  Host scalar of the
 * call: omd = 1.f - decay.  Per element i:
 *     decay == 0    :  ema[i] = params[i]                          a copy of the bits -- -0.0, infinities, NaN payloads and denormals come
 *                                                                  out as they went in; ema is not read (it may hold anything), 8 bytes
 *                                                                  per element
 *     averaged(i)   :  ema[i] = decay * ema[i] + omd * params[i]   two products and one sum, 12 bytes per element
 *     otherwise     :  ema[i] = params[i]                          a copy of the bits: BatchNorm2D's moving statistics, which are
 *                                                                  averages already and follow the model
 * averaged(i): i lies inside one of n_ranges half-open index ranges; avg_ranges, avg_ranges_dev and n_ranges follow the conventions
 * of cnn_sgd_momentum_update's decay_ranges / decay_ranges_dev -- a HOST array of begin, end pairs relative to `params`, ascending,
 * non-empty and disjoint, end <= n; up to CNN_SGD_INLINE_RANGES ranges travel in the kernel arguments, beyond that the kernel reads
 * the DEVICE copy; n <= 2^32 - 257.  With n_ranges == 0 no element is averaged and the call is the copy.  ema and params may be
 * misaligned independently (a pointer that is not 16-byte aligned, or n < 4, takes the scalar kernel, same results).  Checked before
 * any launch: no null pointer, n > 0, ema and params do not overlap, decay in [0, 1) (a NaN fails), the range table.  One kernel
 * launch per call (its name begins with ema_).
 * cnn_ema_decay_at: the decay of the update that follows updates_done earlier ones -- pure host code.  warmup == 0: decay.
 * Otherwise min(decay, (float)((1.0 + t) / (10.0 + t))) with t = (double)updates_done: the warm-up of TF and timm, whose first
 * update uses 0.1. */
float cnn_ema_decay_at(float decay, int warmup, uint64_t updates_done);
int cnn_ema_update(float* ema, const float* params, size_t n, float decay, const uint32_t* avg_ranges, const uint32_t* avg_ranges_dev,
                   size_t n_ranges, void* stream);

/* Exchanges the bits of two disjoint buffers of n floats in one launch (its name begins with aswap_): 16 bytes per element, any
 * alignment, every bit pattern survives; two calls restore both buffers.  Checked before the launch: no null pointer, n > 0, a and b
 * at least n floats apart. */
int cnn_arena_swap(float* a, float* b, size_t n, void* stream);

/* ---- layer-wise optimizers: LAMB and LARS over one flat arena cut into tensors ("segments") --------------------------------------
 * A handle describes how the flat range [0, n) is cut into n_segments tensors and owns the device copy of that table, the workspace
 * of the segmented norm and a device statistics array; it is created once and reused every step (no per-step host-to-device copy).
 *   seg_bounds : HOST array of n_segments + 1 values, seg_bounds[0] = 0, strictly ascending, the last one is n (<= 2^32 - 257)
 *   seg_flags  : HOST array of n_segments values, any of CNN_SEG_DECAY | CNN_SEG_ADAPT
 * Both are checked; a bad table is an error status with a message and nothing is allocated.
 *
 * Segment norms: norm[s] = (float)sqrt( sum over the segment of (double)x[i] * (double)x[i] ).  The flat range is cut into chunks of
 * CNN_SEG_CHUNK elements, one workgroup each; a workgroup reduces every (segment, chunk) overlap separately into that overlap's own
 * fp64 slot, a finish kernel adds each segment's slots in ascending order.  No floating-point atomics, and the order of every sum
 * depends on the table alone -- not on the grid, not on the pointers' alignment: the same words from run to run.  Two launches.
 *
 * cnn_lamb_update (You et al., "Large Batch Optimization for Deep Learning"), in cnn_adam_update's arithmetic: fp32, every product,
 * sum, quotient and root rounded separately (no FMA), quotients and roots correctly rounded, denormals kept.  Host scalars:
 *     omb1 = 1.f - beta1, omb2 = 1.f - beta2 (fp32)     bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step))
 *     bc1  = (float)(1.0 - pow((double)beta1, (double)step))
 * Per element i of segment s:
 *     gs  = grad_scale != 1 ? g * grad_scale : g
 *     m'  = beta1 * m + omb1 * gs          v' = beta2 * v + omb2 * (gs * gs)
 *     den = sqrt(v') / bc2s + eps          mh = m' / bc1          q = mh / den
 *     r   = (DECAY(s) && weight_decay != 0) ? q + weight_decay * p : q                    (update[i] receives r)
 *     w_norm[s] = norm of p (before the step) over s ;  u_norm[s] = norm of r over s
 *     ratio[s]  = (ADAPT(s) && w_norm[s] > 0 && u_norm[s] > 0) ? w_norm[s] / u_norm[s] : 1
 *     t = ratio[s] * r ;  p' = p - lr * t ;  previous[i] = p   (previous is nullable)
 * exp_avg (m), exp_avg_sq (v), params are written, grads is not.  Three launches: moments + r + the partial sums of both norms in
 * one pass (28 B per element), the finish, the apply pass (12 B per element, 16 with previous).
 *
 * cnn_lars_update (You et al., "Large Batch Training of Convolutional Networks") on cnn_sgd_momentum_update's arithmetic:
 *     gs as above;  g_norm[s] = norm of g over s;  gnt = grad_scale != 1 ? g_norm[s] * grad_scale : g_norm[s]   (stored as u_norm[s])
 *     wds = DECAY(s) ? weight_decay : 0
 *     ratio[s] = (ADAPT(s) && w_norm[s] > 0 && gnt > 0) ? (trust_coefficient * w_norm[s]) / ((gnt + wds * w_norm[s]) + eps) : 1
 *     d  = (DECAY(s) && weight_decay != 0) ? gs + weight_decay * p : gs ;   dl = ratio[s] * d
 *     momentum == 0 :  u = dl        otherwise :  v' = momentum * v + dl ;  u = nesterov ? dl + momentum * v' : v'
 *     p' = p - lr * u
 * With no CNN_SEG_ADAPT flag in the table every ratio is exactly 1 and the result equals cnn_sgd_momentum_update's, with the DECAY
 * segments as its ranges, bit for bit.  Three launches: the partial sums of both norms (8 B per element), the finish, the step (20 B
 * per element, 24 with previous).
 *
 * Both: the host never waits and nothing is copied; pointers that are not 16-byte aligned take scalar loads and stores with the
 * same results.  Checked before any launch: the handle, null pointers, beta1, beta2 in [0, 1), eps > 0, weight_decay >= 0,
 * momentum >= 0, trust_coefficient > 0, step >= 1.  cnn_layerwise_stats: device pointer to 3 * n_segments floats of the latest update
 * call -- w_norm[s], then u_norm[s], then ratio[s] (three arrays). */
#define CNN_SEG_DECAY 1u   /* weight decay applies to this segment */
#define CNN_SEG_ADAPT 2u   /* the trust ratio applies to this segment (otherwise its ratio is exactly 1) */
#define CNN_SEG_CHUNK 1024
int cnn_layerwise_create(const uint32_t* seg_bounds, const uint32_t* seg_flags, size_t n_segments, void** handle);
int cnn_layerwise_destroy(void* handle);
int cnn_layerwise_stats(void* handle, float** stats_dev);
int cnn_segment_norms(void* handle, const float* x, float* norms_dev, void* stream);
typedef struct cnn_lamb_options {
    float lr, beta1, beta2, eps, weight_decay;
    uint64_t step;        /* 1-based number of THIS step */
} cnn_lamb_options;
int cnn_lamb_update(void* handle, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* update /* n floats of scratch */,
                    const cnn_lamb_options* opt, float grad_scale, float* previous /* nullable */, void* stream);
typedef struct cnn_lars_options {
    float lr, momentum, weight_decay, trust_coefficient, eps;
    int nesterov;         /* 0 / 1 */
} cnn_lars_options;
int cnn_lars_update(void* handle, float* params, const float* grads, float* velocity /* NULL allowed when momentum == 0 */,
                    const cnn_lars_options* opt, float grad_scale, float* previous /* nullable */, void* stream);

/* AlexNet::grad_cam (alexnet.cpp:107-140) from the feature map of the chosen layer, [B][C][H][W] on the device:
 *   weights[b][o] = mean_i feature[b][o][i];  cam[b] = ReLU(sum_o weights[b][o] * feature[b][o]);  cam = (cam - min) / (max - min)
 * with min / max over the whole [B][H][W] tensor (:136-139).  cam: [B][H][W] floats (output).  image (nullable): H*W bytes, the 8-bit
 * picture of the FIRST plane -- what the reference returns as cv::Mat through Tensor3D::opecv_mat(1) (data_format.cpp:98-103). */
int cnn_grad_cam(const float* feature, int B, int C, int H, int W, float* cam, unsigned char* image, void* stream);

/* ---- data-parallel gradient exchange (new: the reference is single-process) -------------
 * The batch is sharded over G replicas (one per GPU); the only cross-sample coupling of the path is the batch mean inside
 * the weight / bias gradients (conv2d.cpp:148,157; linear.cpp:62,70).  Every replica's kernels divide by their LOCAL batch,
 * cnn_allreduce_grads sums the flat gradient arena (or one bucket of it) in place over the replicas -- RCCL ncclAllReduce,
 * fp32 sum, over xGMI -- and cnn_sgd_update(..., grad_scale = 1/G) folds the rest: exactly the reference's (1/B) * sum over the
 * whole batch up to summation order.  BatchNorm2D gamma / beta gradients computed by the sync-BN entry points are already
 * full-batch sums on every replica; summing them over G and scaling by 1/G leaves them unchanged, so they ride in the same
 * arena.  librccl is bound at run time (dlopen("librccl.so.1")): libcnn_amd.so has no link-time dependency on it.
 *   one process per GPU : rank 0 calls cnn_comm_unique_id, ships the 128 bytes to the other ranks by any means (the test
 *                         harness uses torch.distributed's store), every rank calls cnn_comm_init_rank on its device;
 *   one process, n GPUs : cnn_comm_init_all (ncclCommInitAll), one host thread per device or cnn_comm_group_start/_end
 *                         around the per-device calls. */
#define CNN_COMM_ID_BYTES 128
int cnn_comm_available(void); /* != 0: librccl was found and bound */
int cnn_comm_version(void);   /* ncclGetVersion code, 0 when unavailable */
int cnn_comm_unique_id(void* id_out /* host, CNN_COMM_ID_BYTES */);
int cnn_comm_init_rank(void** comm, int world, int rank, const void* id /* host, CNN_COMM_ID_BYTES */);
int cnn_comm_init_all(void** comms /* [ndev] */, int ndev, const int* devices /* NULL = 0..ndev-1 */);
int cnn_comm_info(void* comm, int* world, int* rank);
int cnn_comm_destroy(void* comm);
int cnn_comm_group_start(void);
int cnn_comm_group_end(void);
/* in-place sum of n floats over all ranks of comm, enqueued on `stream` */
int cnn_allreduce_grads(void* comm, float* grads, size_t n, void* stream);
/* a second communicator over the same ranks (ncclCommSplit; every rank calls it with the same color, key orders the ranks): collectives
 * on different communicators are independent queues, so BatchNorm2D's small sync-BN reductions (batchnorm2d.cpp:46-61, 129-147) need not
 * queue behind the bucketed gradient exchange.  Fails with CNN_AMD_E_COMM when the bound librccl has no ncclCommSplit. */
int cnn_comm_split(void* comm, int color, int key, void** new_comm);
/* `bytes` bytes at buf (device) of rank `root` to every rank of comm, in place, enqueued on `stream` */
int cnn_comm_broadcast(void* comm, void* buf, size_t bytes, int root, void* stream);

/* ---- loss glue : func.cpp:16-73 (caller side of the path; keeps the step on the device) -------------- */
/* probs = softmax(logits) with the reference's clamped exp and NaN->0; delta = probs - onehot(labels);
 * loss_sum[0] = -sum_b log(probs[b][label_b])  (the caller divides by the global batch, func.cpp:67,71).
 * probs / loss_sum may be NULL. */
int cnn_softmax_xent(const float* logits, const int32_t* labels, float* probs, float* delta, float* loss_sum,
                     int B, int classes, void* stream);
/* LinearLayer::forward of the last layer + cnn_softmax_xent in ONE kernel (out <= 8): logits, probs (nullable), delta as
 * above, and the per-sample loss term log(probs[b][label_b]) into loss_terms[b]; cnn_loss_from_terms adds the terms in
 * ascending sample order (the reference's order) whenever the loss value is actually wanted.  Bit-identical to
 * cnn_linear_forward + cnn_softmax_xent. */
int cnn_linear_forward_softmax_xent(const float* x, const float* w, const float* bias, const int32_t* labels, float* logits,
                                    float* probs, float* delta, float* loss_terms, int B, int in, int out, void* stream);
/* ... and the data gradient of that layer in the same kernel: dx[b][i] = sum_j delta[b][j] * W[i][j] (linear.cpp:73-90; a sample's row
 * needs only that sample's delta), relu_below != 0: followed by the ReLU::backward of the layer whose output is x (x <= 0 ? 0 : dx).
 * Bit-identical to cnn_linear_forward_softmax_xent + the dx of cnn_linear_backward(_relu).  The layer's weight / bias gradient (which
 * needs every sample's delta) is cnn_linear_backward(x, delta, w, gw, gb, NULL, ...): with dx == NULL it runs the same summation
 * order as the three-output call, on any stream -- a train step then has ONE kernel between its last forward convolution and its
 * first data gradient. */
int cnn_linear_forward_softmax_xent_dx(const float* x, const float* w, const float* bias, const int32_t* labels, float* logits,
                                       float* probs, float* delta, float* loss_terms, float* dx, int relu_below, int B, int in, int out,
                                       void* stream);
int cnn_loss_from_terms(const float* loss_terms, float* loss_sum, int B, void* stream);

/* ---- soft targets: label smoothing, mixup and CutMix on the device --------------------------------------------------------------
 * The partner rule shared by cnn_soft_targets and cnn_batch_mix: which sample p(b) of the same batch sample b is mixed with.  It takes no
 * index array, so the host checks it:
 *     CNN_PAIR_NONE :  no partner
 *     CNN_PAIR_FLIP :  p(b) = B - 1 - b            (timm; pair_shift is ignored; the middle sample of an odd batch is its own partner and
 *                                                   goes through the same arithmetic as any other)
 *     CNN_PAIR_ROLL :  p(b) = (b + shift) % B      with 1 <= shift < B (torchvision: shift 1) */
enum { CNN_PAIR_NONE = 0, CNN_PAIR_FLIP = 1, CNN_PAIR_ROLL = 2 };

/* Dense target rows from labels: targets[B][classes] for the soft loss entries below.  fp32, every operation rounded separately, no FMA.
 * Host scalars of the call:   u = smoothing / (float)classes     hot = (1.f - smoothing) + u     oml = 1.f - lam
 *     base(l, j) = smoothing == 0 ? (j == l ? 1.f : 0.f) : (j == l ? hot : u)
 *     pair_rule == CNN_PAIR_NONE or lam == 1 :  targets[b][j] = base(labels[b], j)
 *     otherwise                              :  targets[b][j] = lam * base(labels[b], j) + oml * base(labels[p(b)], j)
 *                                                                two products and one sum
 * A label outside [0, classes) matches no j, as in the hard-label kernels; the labels are device memory and are not checked.  Checked
 * before the launch: no null pointer, B > 0, classes > 0, smoothing in [0, 1) and lam in [0, 1] (a NaN fails either), a known rule, a
 * ROLL shift in [1, B).  One small launch (its name begins with soft_targets). */
int cnn_soft_targets(const int32_t* labels, float* targets /* [B][classes] */, int B, int classes, float smoothing, float lam,
                     int pair_rule, int pair_shift, void* stream);

/* mixup / CutMix of a contiguous NCHW batch with its partner samples, OUT OF PLACE: dst and src must not overlap (checked; a partner
 * read beside an in-place write would be a race), src is not written.  One launch (its name begins with bmix_).
 *     CNN_MIX_MIXUP  :  dst[b][e] = lam * src[b][e] + oml * src[p(b)][e]        oml = 1.f - lam on the host; fp32, two products and one
 *                                                                               sum, each rounded, no FMA, denormals kept; 12 bytes per
 *                                                                               element
 *     CNN_MIX_CUTMIX :  dst[b][c][y][x] = (y0 <= y < y1 && x0 <= x < x1) ? src[p(b)][c][y][x] : src[b][c][y][x]
 *                                                                               a copy of the bits, lam is ignored (cnn_cutmix_lambda gives
 *                                                                               the box's); 16-byte groups wholly inside or outside the box
 *                                                                               request one source only: towards 8 bytes per element
 * pair_rule == CNN_PAIR_NONE, MIXUP with lam == 1 and CUTMIX with an empty box are the copy of the bits (as cnn_ema_update at decay 0):
 * -0.0, infinities, NaN payloads and denormals come out as they went in.  Any pointer alignment and any sample size: the float4 kernels
 * run when both pointers are 16-byte aligned and C*H*W % 4 == 0 (every sample, hence every partner, then starts aligned), the scalar
 * kernels otherwise, same results.  Checked before the launch: no null pointer, B, C, H, W > 0, C*H*W < 2^31, a known mode and rule, a ROLL
 * shift in [1, B), MIXUP: lam in [0, 1] (a NaN fails), CUTMIX: 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W (an empty box is a copy). */
enum { CNN_MIX_MIXUP = 1, CNN_MIX_CUTMIX = 2 };
typedef struct cnn_mix_desc {
    int mode;                  /* CNN_MIX_MIXUP | CNN_MIX_CUTMIX */
    float lam;                 /* MIXUP: weight of the sample itself */
    int pair_rule, pair_shift; /* CNN_PAIR_* */
    int y0, y1, x0, x1;        /* CUTMIX: the box [y0, y1) x [x0, x1) of every plane that comes from the partner */
} cnn_mix_desc;
int cnn_batch_mix(const cnn_mix_desc* d, const float* src, float* dst, int B, int C, int H, int W, void* stream);
/* the weight of the sample itself under a CutMix box: (float)(1.0 - (double)((y1 - y0) * (x1 - x0)) / ((double)H * W)) -- pure host code */
float cnn_cutmix_lambda(int H, int W, int y0, int y1, int x0, int x1);

/* cnn_softmax_xent, cnn_linear_forward_softmax_xent and cnn_linear_forward_softmax_xent_dx against a dense target tensor
 * targets[B][classes] (fp32, e.g. from cnn_soft_targets) instead of labels: yv = targets[b][i] takes the place of (i == label ? 1 : 0)
 * and nothing else changes -- delta[b][i] = probs[b][i] - yv, the sample's loss term is sum_i logf(probs[b][i]) * yv in ascending i
 * (the reference's log(0) * 0 = NaN included), same kernels, same order.  A one-hot target tensor therefore reproduces the hard-label
 * entry bit for bit in logits, probs, delta, loss terms and dx. */
int cnn_softmax_xent_soft(const float* logits, const float* targets, float* probs, float* delta, float* loss_sum, int B, int classes,
                          void* stream);
int cnn_linear_forward_softmax_xent_soft(const float* x, const float* w, const float* bias, const float* targets, float* logits,
                                         float* probs, float* delta, float* loss_terms, int B, int in, int out, void* stream);
int cnn_linear_forward_softmax_xent_soft_dx(const float* x, const float* w, const float* bias, const float* targets, float* logits,
                                            float* probs, float* delta, float* loss_terms, float* dx, int relu_below, int B, int in,
                                            int out, void* stream);

/* ---- evaluation on the device: loss, top-1 / top-k and confusion counts without a host round trip per batch ----------------------
 * The evaluation state is ONE device block whose all-zero bytes are the empty state (clear it with cnn_memset_zero); its layout, 8-byte
 * words throughout, cnn_eval_state_bytes(classes) = 8 * (4 + 1 + classes * classes) bytes:
 *     uint64 counts[4]                     samples, top-1 correct, top-k correct, ignored
 *     double loss_sum                      running sum of the batch loss sums
 *     uint64 confusion[classes][classes]   row = label, column = prediction
 * cnn_eval_accumulate adds one batch of logits [B][classes] to it in ONE launch (its name begins with eval_).  Per sample b with logits z
 * and label y:
 *     prediction : the first maximum, strict '>' starting at index 0 (Tensor3D::argmax, the max loop of cnn_softmax_xent); written to
 *                  pred[b] when pred is given, for ignored samples too.  A NaN is never greater: a NaN at index 0 stays the prediction,
 *                  a NaN elsewhere is never one.
 *     ignored    : a label outside [0, classes) counts in `ignored` ONLY -- nothing in samples, top-1, top-k, confusion or the loss (a
 *                  padded last batch: label -1).
 *     top-1      : pred == y.            confusion[y][pred] += 1.
 *     top-k      : rank < k with rank = #{j : z[j] > z[y]} + #{j < y : z[j] == z[y]} (ties go to the lower index, as in the
 *                  prediction: on rows without NaN rank == 0 is the same as pred == y).
 *     loss term  : logf(p[y]) with exactly cnn_softmax_xent's per-sample expressions in its order -- sequential max, sequential sum of the
 *                  clamped exp of z[i] - max, p = clamped_exp(z[y] - max) / sum, NaN -> 0.
 *     batch sum  : the terms of the non-ignored samples added in ascending sample order in fp32, negated: with no label out of range
 *                  it has the bits of cnn_softmax_xent's loss_sum[0] (while no probability of the row underflows to 0, where that entry's
 *                  log(0) * 0 gives NaN and this one does not).
 *     running    : loss_sum += (double)batch_sum, once per launch.
 * The counts are integer adds.  Nothing depends on a launch shape: the same calls give the same bytes.  The labels are device memory and
 * are not checked on the host.  Checked before the launch: no null pointer except pred, B > 0, classes > 0, 1 <= k <= classes.
 * cnn_eval_read is the one call that copies back and synchronises: counts and loss into *out, the confusion matrix into `confusion`
 * (host, classes * classes values) when it is given.  mean loss = loss_sum / samples, accuracy = top1 / samples. */
typedef struct cnn_eval_result {
    uint64_t samples, top1, topk, ignored;
    double loss_sum;
} cnn_eval_result;
size_t cnn_eval_state_bytes(int classes); /* pure host code; 0 and a message for classes <= 0 */
int cnn_eval_accumulate(const float* logits, const int32_t* labels, int32_t* pred /* [B], nullable */, void* state, int B, int classes, int k,
                        void* stream);
int cnn_eval_read(const void* state, int classes, cnn_eval_result* out, uint64_t* confusion /* nullable, host */, void* stream);

/* ---- device memory / transfer helpers (the host layer classes use only these) ------------------------ */
int cnn_device_alloc(void** ptr, size_t bytes);
int cnn_device_free(void* ptr);
int cnn_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream); /* async on stream */
int cnn_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream); /* async on stream */
int cnn_memcpy_d2d(void* dst_dev, const void* src_dev, size_t bytes, void* stream);
int cnn_memset_zero(void* dst_dev, size_t bytes, void* stream);
int cnn_stream_synchronize(void* stream);
/* streams / events for callers that overlap independent work themselves (the communication stream of the data-parallel
 * exchange, the staging stream of cnn_batch_upload_async); streams are non-blocking w.r.t. the default stream, events carry
 * no timing.  The host layer classes use only these, never the HIP runtime directly. */
int cnn_stream_create(void** stream);
/* level < 0: the device's highest stream priority, 0: default, > 0: lowest (hipStreamCreateWithPriority; dispatch arbitration between
 * queues, running waves are not preempted) */
int cnn_stream_create_priority(void** stream, int level);
int cnn_stream_destroy(void* stream);
int cnn_event_create(void** event);
int cnn_event_destroy(void* event);
int cnn_event_record(void* event, void* stream);
int cnn_stream_wait_event(void* stream, void* event);
/* like cnn_stream_wait_event, for a dependency that only concerns work queued on `stream` ITSELF: the caller asserts that nothing the
 * library forks off `stream` afterwards (the weight-gradient side stream of cnn_conv2d_backward*) depends on the event, so a fork
 * point published by the last kernel (cnn_amd_publish_next_kernel) stays valid.  cnn_stream_wait_event invalidates it. */
int cnn_stream_wait_event_local(void* stream, void* event);
/* ---- input staging (row n4: what DataLoader::generate_batch's host buffers -- pipeline.cpp:112-140 -- need in front of a device
 * consumer).  A stager owns `depth` (>= 2) page-locked host slots and as many device buffers of batch_bytes each, a copy stream
 * and the events that order producer -> H2D -> consumer -> producer:
 *   acquire(&host, &slot)   the pinned slot to fill next; BLOCKS (host) until the consumer released it from its previous use
 *   submit(slot, &dev)      enqueue the H2D copy of that slot on the stager's own stream; dev = its device buffer
 *   wait(slot, stream)      make `stream` wait for that copy (enqueue only)
 *   release(slot, stream)   `stream` is done reading the device buffer: the slot may be overwritten once it gets there
 * so that the upload of batch i+1 overlaps the kernels of batch i.  A batch of 256 x 3 x 224 x 224 floats is 154 MB: ~2.4 ms
 * over PCIe Gen5 x16, i.e. the PCIe-inclusive ceiling of the reference net is ~10^5 images/s per GPU (bench.py --staged-input). */
int cnn_batch_stager_create(void** stager, size_t batch_bytes, int depth);
/* The same for what a real input is BEFORE Tensor3D::read_from_opencv_mat (data_format.cpp:13-23): B images of H x W x 3 interleaved
 * bytes (cv::Mat CV_8UC3, channel order as it lies -- BGR for cv::imread).  The pinned slots and the H2D copies hold BYTES (a quarter
 * of the fp32 batch: 150 KB instead of 602 KB per 224 x 224 image); behind the copy, still on the stager's own stream, one kernel
 * writes the batch the layers consume -- fp32, planar [B][3][H][W], data[c*H*W + i] = byte * 1.f / 255 through a 256-entry table that
 * the HOST fills with that very expression, so the result is bit-identical to the reference's conversion.  Any H, W (pixel counts that
 * are multiples of four take the 16-byte-store kernel).  submit() returns the fp32 batch; acquire / wait / release / destroy as above. */
int cnn_batch_stager_create_u8(void** stager, int B, int H, int W, int depth);
int cnn_batch_stager_destroy(void* stager);
int cnn_batch_stager_acquire(void* stager, void** pinned_host, int* slot);
int cnn_batch_stager_submit(void* stager, int slot, void** device_ptr);
int cnn_batch_stager_wait(void* stager, int slot, void* stream);
int cnn_batch_stager_release(void* stager, int slot, void* stream);

/* ---- geometric augmentation of uint8 batches on the device (an addition: ImageAugmentor, pipeline.cpp:40-77, runs OpenCV on the host).
 * Flip, crop, rotate and the resize to the network's size are ONE affine map per sample; one kernel gathers through it while it does the
 * stager's bytes -> fp32 planar conversion.  Decode is not covered.  The gather takes two taps per axis whatever the map's scale: a shrink
 * ratio of 2 or more aliases, except out of a resident dataset that keeps half-size levels (cnn_dataset_create_u8_levels below).  Colour
 * jitter, normalisation and erasing: the photo stager below.
 * The rule.  Input: interleaved bytes [B][Hs][Ws][3]; output: planar fp32 [B][3][H][W].  Sample b has six floats m[b][0..5] that map
 * OUTPUT pixel indices to SOURCE pixel indices.  Per output pixel (x, y), all in fp32, every product and sum rounded separately:
 *     sx = (m0*x + m1*y) + m2            sy = (m3*x + m4*y) + m5
 *     inside = sx >= -0.5f && sx <= Ws-0.5f && sy >= -0.5f && sy <= Hs-0.5f
 *     x0f = floorf(sx); fx = sx - x0f;   y0f = floorf(sy); fy = sy - y0f
 *     x0 = clamp((int)x0f, 0, Ws-1); x1 = clamp((int)x0f + 1, 0, Ws-1)      (same for y)
 *     t.. = lut[byte]                    (the stager's table: v * 1.f / 255 computed on the host)
 *     top = t00 + fx*(t01 - t00); bot = t10 + fx*(t11 - t10); out = top + fy*(bot - top)
 *     out = inside ? out : fill
 * A position inside the source's pixel area reads edge-replicated taps (a resize), a position outside it gives `fill` (the constant
 * border of a rotation's corners).  With fx == 0 the rule yields t00 exactly: the identity, flips, integer shifts and quarter turns are
 * bit-identical to the plain conversion of the permuted image.  tests/augment_ref.py restates the rule in NumPy; the kernel equals it
 * bit for bit.
 * cnn_augment_u8: one launch per batch.  Checked before it: no null pointer, B and every dimension in 1..8192 (fp32 holds those indices
 * exactly), a finite fill.  The matrices are device memory and are not checked on the host; a non-finite entry gives `fill`. */
int cnn_augment_u8(const unsigned char* src, int B, int Hs, int Ws, const float* matrices_dev /* [B][6] */, float fill, float* dst, int H, int W,
                   void* stream);
/* cnn_augment_matrix composes such a map on the host (no GPU call).  The ops apply in order to a canvas that starts as the source, the way
 * ImageAugmentor::make_augment transforms its cv::Mat: HFLIP / VFLIP mirror the canvas, CROP (a, b, c, d = x0, y0, w, h in the current
 * canvas) shrinks it, ROTATE (a = degrees, positive = counter-clockwise on the screen as cv::getRotationMatrix2D) turns it about its
 * centre ((cw-1)/2, (ch-1)/2) and keeps its size.  Last comes the resize of the canvas to W x H with half-pixel centres,
 * sx = (x + 0.5) * cw / W - 0.5.  Composed in double, rounded to fp32 once.  Rotations by multiples of 90 degrees take sine and cosine
 * from a table (integers map to integers); n_ops == 0 with equal sizes gives exactly {1,0,0, 0,1,0}.  Rejected: a crop box outside the
 * current canvas, unknown kinds, non-finite arguments, dimensions outside 1..8192. */
enum { CNN_AUG_HFLIP = 1, CNN_AUG_VFLIP = 2, CNN_AUG_CROP = 3, CNN_AUG_ROTATE = 4 };
typedef struct cnn_augment_op {
    int kind;
    float a, b, c, d;
} cnn_augment_op;
int cnn_augment_matrix(const cnn_augment_op* ops, int n_ops, int Hs, int Ws, int H, int W, float m[6]);
/* The u8 stager with that kernel in place of the plain conversion: a slot holds B images of Hs x Ws x 3 bytes and B * 6 pinned floats.
 * acquire() presets the slot's matrices to the plain resize map (the identity when the sizes are equal), so a caller who does not touch
 * them gets the plain conversion; cnn_batch_stager_matrices() hands out the slot's pinned block to overwrite between acquire() and
 * submit().  submit() uploads bytes and matrices and runs cnn_augment_u8, all on the stager's stream in front of the event wait() waits
 * for; it returns the fp32 [B][3][H][W] batch.  cnn_batch_stager_set_fill: the border value of later submits (default 0).  Both return
 * CNN_AMD_E_BADARG on a stager of the other two kinds. */
int cnn_batch_stager_create_u8_aug(void** stager, int B, int Hs, int Ws, int H, int W, int depth);
int cnn_batch_stager_matrices(void* stager, int slot, float** pinned /* [B][6] */);
int cnn_batch_stager_set_fill(void* stager, float fill);

/* ---- the photometric half on the device: colour jitter, mean / std normalisation and random erasing in the same kernel, on the three
 * channel values of an output pixel right before the store (no extra pass over memory).  Reached through a photo stager only.
 * The rule.  Sample b has 20 floats p[b][0..19]; the stager has s[3], t[3] and a clamp flag.  Per output pixel (x, y), behind the gather
 * rule above, all in fp32, every product and sum rounded separately:
 *     v0,v1,v2 = the gather rule's three channel values of this pixel (inside pixels only)
 *     u_c   = ((A[c][0]*v0 + A[c][1]*v1) + A[c][2]*v2) + o[c]        A = p[0..8] row-major, o = p[9..11]
 *     u_c   = clamp ? fminf(fmaxf(u_c, 0), 1) : u_c
 *     out_c = u_c * s[c] + t[c]                                      (normalisation: s = 1/std, t = -mean/std)
 *     out_c = inside ? out_c : fill                                  (fill is in OUTPUT units: the colour stage does not touch it)
 *     ex0,ey0,ew,eh = p[12..15] (whole numbers), ev[c] = p[16..18], p[19] reserved = 0
 *     out_c = (ex0 <= x && x < ex0+ew && ey0 <= y && y < ey0+eh) ? ev[c] : out_c     (fp32 comparisons; ev in output units)
 * ew == 0 or eh == 0 is no box; a box that runs past the output is clipped by the comparisons.  One box per sample, one value per
 * channel: per-pixel noise is not covered.  With A = I, o = 0, clamp off, s = 1, t = 0 and no box the rule returns the gather rule's
 * bits unchanged (the table holds finite values >= 0: 1*v + 0*w == v).  tests/photo_ref.py restates the rule in NumPy; the kernel equals
 * it bit for bit.  The parameters are pinned memory the caller writes and cannot be checked: a non-finite one gives unspecified pixels,
 * never an access out of bounds.
 * cnn_batch_stager_create_u8_photo: an augmenting stager (cnn_batch_stager_matrices and _set_fill work on it) whose slots carry a pinned
 * [B][20] block as well; acquire() presets it to the identity above, cnn_batch_stager_photo() hands it out to overwrite between
 * acquire() and submit(), submit() uploads it with the matrices and runs the kernel on the stager's stream in front of the event wait()
 * waits for.  cnn_batch_stager_set_normalize: s = 1/std and t = -mean/std of LATER submits, computed in double and rounded once; std
 * finite and non-zero, mean finite; clamp != 0 turns the clamp to [0, 1] on.  Default: s = 1, t = 0, clamp off.  Both return
 * CNN_AMD_E_BADARG on a stager of the other kinds. */
int cnn_batch_stager_create_u8_photo(void** stager, int B, int Hs, int Ws, int H, int W, int depth);
int cnn_batch_stager_photo(void* stager, int slot, float** pinned /* [B][20] */);
int cnn_batch_stager_set_normalize(void* stager, const float mean[3], const float std[3], int clamp);
/* cnn_colour_matrix composes A and o on the host (no GPU call): out[0..8] = A row-major, out[9..11] = o, the first twelve floats of a
 * sample's block.  The ops apply in order to a colour x in [0, 1]^3, each an affine map, composed in double and rounded to fp32 once:
 *   CNN_COL_BRIGHTNESS  a = f          x * f
 *   CNN_COL_CONTRAST    a = f, b = pivot   f * x + (1 - f) * pivot.  The pivot is FIXED (0.5, or the dataset's mean grey): torchvision's
 *                       ColorJitter uses the mean grey of each image, which would need a second pass over it.
 *   CNN_COL_SATURATION  a = f          f * x + (1 - f) * gray(x), gray = 0.299 r + 0.587 g + 0.114 b
 *   CNN_COL_HUE         a = degrees    a rotation about the grey axis in YIQ (I' = cos*I - sin*Q, Q' = sin*I + cos*Q): the LINEAR form of
 *                       a hue shift, not torchvision's HSV one (they agree on saturated primaries' direction, not in value).
 *                       Multiples of 90 degrees take sine and cosine from a table: 360 is 0 exactly.
 * There is NO clamp between the ops, only the one clamp of the kernel behind the whole map: where torchvision clamps after every op, a
 * value that leaves [0, 1] in between comes back differently here.  n_ops == 0 gives I and 0.  Rejected: unknown kinds, non-finite
 * arguments, a composed map that is not finite. */
enum { CNN_COL_BRIGHTNESS = 1, CNN_COL_CONTRAST = 2, CNN_COL_SATURATION = 3, CNN_COL_HUE = 4 };
typedef struct cnn_colour_op {
    int kind;
    float a, b;
} cnn_colour_op;
int cnn_colour_matrix(const cnn_colour_op* ops, int n_ops, float out[12]);

/* ---- a device-resident uint8 dataset: decode once, upload once, gather every batch by index out of HBM (an addition: the reference's
 * DataLoader decodes and resizes every image again every epoch, pipeline.cpp:112-140).  What crosses PCIe per batch is then B indices and
 * B * 26 floats instead of B * Hs * Ws * 3 bytes.
 * cnn_dataset_create_u8: N images of Hs x Ws x 3 interleaved bytes (N * Hs * Ws * 3 bytes, may exceed 4 GiB: every offset into the store
 * is 64-bit) and N int32 labels on the CURRENT device; N in 1 .. 2^31-1, Hs and Ws in 1 .. 8192.  Every image byte starts as 0 and every
 * label as -1: no uninitialised byte can reach a result.
 * cnn_dataset_write / _read: samples [first, first + count) from / to PAGEABLE or pinned host memory; images [count][Hs][Ws][3] and
 * labels [count], either may be NULL (that part is left alone), not both.  Blocking host calls: they return when the data is on the
 * device / on the host.  write() first waits, on the host, until every gather that a stager attached to this dataset has already
 * submitted has finished (it synchronises their copy streams): a submitted batch always holds the bytes that were there at submit(), a
 * later submit always sees the write, and the caller has no rule to follow.  Rejected: count <= 0, a range that leaves [0, N), both
 * pointers NULL.
 * cnn_dataset_info: N, Hs, Ws (each pointer may be NULL, not all three).
 * cnn_dataset_destroy: CNN_AMD_E_BADARG, and nothing changed, while a stager is attached (destroy the stagers first); NULL is refused. */
int cnn_dataset_create_u8(void** dataset, long long N, int Hs, int Ws);
int cnn_dataset_write(void* dataset, long long first, long long count, const unsigned char* images /* host [count][Hs][Ws][3], nullable */,
                      const int* labels /* host [count], nullable */);
int cnn_dataset_read(void* dataset, long long first, long long count, unsigned char* images /* nullable */, int* labels /* nullable */);
int cnn_dataset_info(void* dataset, long long* N, int* Hs, int* Ws);
int cnn_dataset_destroy(void* dataset);
/* The fourth kind of u8 stager: a photo stager (cnn_batch_stager_matrices, _photo, _set_fill and _set_normalize work on it unchanged)
 * whose source is the dataset.  A slot has NO pinned image block and no device byte block; it carries one pinned block of B int32 indices
 * followed by the B * 26 floats, a device copy of that block, the fp32 [B][3][H][W] output and a device int32 [B] label buffer.
 * The rule, added to the gather rule and the photometric rule above with nothing else changed: sample b reads idx = indices[b]; its
 * source image is sample idx of the store; with idx == -1 no pixel of the sample is inside and no byte of the store is read (every pixel
 * is `fill`, an erase box still applies); labels_out[b] = idx < 0 ? -1 : labels[idx].  tests/resident_ref.py restates it.
 *   acquire()  returns *pinned_host = NULL; presets the indices to -1, the matrices to the plain resize map, the photo blocks to the identity
 *   cnn_batch_stager_indices()  the slot's pinned [B] indices, to overwrite between acquire() and submit()
 *   submit()   checks the B indices on the host: one outside [-1, N) returns CNN_AMD_E_BADARG with nothing enqueued, and the slot stays
 *              acquired and usable.  Otherwise ONE upload of the block and ONE launch (augment_u8_resident) on the stager's stream in front
 *              of the event wait() waits for; returns the fp32 batch
 *   cnn_batch_stager_labels()   the slot's device label buffer: valid behind the same wait() and until release()
 * cnn_batch_stager_create_u8_resident: B in 1 .. 8192, H and W in 1 .. 8192, depth 2 .. 16; the dataset's device must be the current
 * one; the dataset outlives the stager (cnn_dataset_destroy refuses while it is attached).  _indices and _labels return
 * CNN_AMD_E_BADARG on a stager of the other three kinds. */
int cnn_batch_stager_create_u8_resident(void** stager, void* dataset, int B, int H, int W, int depth);
int cnn_batch_stager_indices(void* stager, int slot, int** pinned /* [B] */);
int cnn_batch_stager_labels(void* stager, int slot, const int** labels_dev /* [B] */);

/* ---- half-size levels for antialiased shrinking out of a resident dataset.  The gather's two taps per axis skip source pixels once the
 * map shrinks by 2 or more.  A dataset made with levels = L > 1 keeps, beside each image, a chain of L - 1 prefiltered half-size images,
 * built once at write time; a stager attached to it picks per sample the level whose residual shrink is below 2, and the gather stays the
 * four-tap kernel with the same traffic per batch.  The store grows by at most a third.
 * The rule.  Levels: level 0 is the image as written, Hs x Ws x 3 interleaved bytes.  Level l has H_l = (H_{l-1} + 1) / 2 and
 * W_l = (W_{l-1} + 1) / 2 (rounded up); its pixel (y, x), channel c, in integers, with p = level l - 1:
 *     y0 = 2y, y1 = min(2y + 1, H_{l-1} - 1), x0 = 2x, x1 = min(2x + 1, W_{l-1} - 1)
 *     v  = (p[y0][x0] + p[y0][x1] + p[y1][x0] + p[y1][x1] + 2) >> 2
 * -- an edge-replicated 2 x 2 box, rounded half up: no floating point, exact on any machine.  The centre of level-l pixel x lies at
 * level-0 coordinate 2^l * (x + 0.5) - 0.5; on an odd size the last pixel is the replicated edge.  L runs from 1 to
 * cnn_dataset_max_levels(Hs, Ws), the number of levels until both dimensions are 1 (at most 14, for 8192).
 * Level choice and level map: host arithmetic in double from the sample's six fp32 floats m, every operation rounded separately:
 *     rx = sqrt(m0*m0 + m3*m3), ry = sqrt(m1*m1 + m4*m4), r = max(rx, ry)      (source pixels per output pixel)
 *     l  = 0; while (l + 1 < L && r >= 2^(l+1)) ++l;                           (rx or ry not finite: l = 0)
 *     l == 0:  m' = m, bit for bit
 *     l  > 0:  m'0,1,3,4 = m0,1,3,4 / 2^l   (exact)
 *              m'2 = (m2 + 0.5) / 2^l - 0.5,  m'5 likewise                     (double, rounded to fp32 once)
 * The residual ratio r / 2^l stays in [1, 2) while levels remain: there the bilinear rule's two taps per axis give every pixel of the
 * level a non-zero weight.  The nearest LOWER level is used; there is no blend between two levels, no anisotropic choice.
 * Gather: sample b with index idx and level l is the gather + photometric + resident rule above, unchanged, applied to image idx of
 * level l with Hs, Ws := H_l, W_l and m := m' (the `inside` test is against the level's size); idx == -1 reads nothing at any level;
 * labels_out as above.  tests/mip_ref.py restates all three parts; the kernels equal it bit for bit.
 * cnn_dataset_max_levels, cnn_augment_level: the two host halves of the rule (no GPU call).  _max_levels returns 0 (and sets the
 * message) for a size outside 1 .. 8192; _augment_level takes levels in 1 .. 14 and writes the level and the six floats of m' (m_level
 * may be m itself).
 * cnn_dataset_create_u8_levels: cnn_dataset_create_u8 with `levels` in 1 .. cnn_dataset_max_levels(Hs, Ws) levels; levels = 1 IS
 * cnn_dataset_create_u8.  One allocation: the level-0 region [N][Hs][Ws][3] first, as ever, then each higher level as [N][H_l][W_l][3];
 * every offset is 64-bit, every byte starts as 0 (the all-zero image's levels are all zero).
 * cnn_dataset_write with images rebuilds, behind the copy, levels 1 .. L-1 of exactly the samples written (one launch of dataset_halve_u8
 * per level on a stream of the dataset's own) and returns when they are done: still a blocking host call, under the same rule about
 * submitted gathers.  A labels-only write launches nothing.  cnn_dataset_read and _info are unchanged (level 0).
 * cnn_dataset_read_level: samples [first, first + count) of one level back to the host, [count][H_l][W_l][3]; blocking.
 * cnn_dataset_level_info: the number of levels and the size of level `level` (each pointer may be NULL, not all three).
 * A resident stager attached to a dataset with L > 1: its slots' pinned block carries, behind the B indices and B * 26 floats, B int32
 * levels and B * 6 level maps (one allocation and one upload still).  submit(), after the index check, runs cnn_augment_level on the
 * caller's maps -- which are not overwritten -- and launches augment_u8_resident_levels in place of augment_u8_resident.
 * cnn_batch_stager_levels hands out the levels the last submit() of that slot chose; CNN_AMD_E_BADARG on the other kinds of stager and
 * on stagers of a one-level dataset.  A stager on a one-level dataset is what it was in every respect. */
int cnn_dataset_max_levels(int Hs, int Ws);
int cnn_augment_level(const float m[6], int levels, int* level, float m_level[6]);
int cnn_dataset_create_u8_levels(void** dataset, long long N, int Hs, int Ws, int levels);
int cnn_dataset_read_level(void* dataset, int level, long long first, long long count, unsigned char* images /* [count][H_l][W_l][3] */);
int cnn_dataset_level_info(void* dataset, int* levels, int level, int* H_l, int* W_l);
int cnn_batch_stager_levels(void* stager, int slot, const int** pinned /* [B] */);

/* page-locked host memory (async H2D / D2H copies are only asynchronous from / to pinned buffers) */
int cnn_host_alloc_pinned(void** ptr, size_t bytes);
int cnn_host_free_pinned(void* ptr);

#ifdef __cplusplus
}
#endif
#endif /* CNN_AMD_H */
