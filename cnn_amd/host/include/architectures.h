// architectures.h -- the reference's layer API (cpu/include/architectures.h:12-138, 196-215) on MI355X.
// Constructors, virtuals and globals keep the reference's names, argument order and defaults; every forward /
// backward / update body is a call into libcnn_amd.so (include/cnn_amd.h).  Errors from the C ABI abort, like the
// reference's asserts (it has no error channel).
#ifndef CNN_AMD_ARCHITECTURES_H
#define CNN_AMD_ARCHITECTURES_H

#include <filesystem>
#include <fstream>
#include <list>
#include <random>
#include <utility>
#include <vector>

#include "data_format.h"

extern "C" {
#include "cnn_amd.h"
}
#include "layer_parts.h"

namespace architectures {

extern data_type random_times;  // init scale divisor (architectures.cpp:6)
extern bool no_grad;            // skip everything only backward needs (architectures.cpp:8)
extern void* stream;            // hipStream_t all layers enqueue on (addition; default stream when null)
// addition: let the AlexNet container run Conv2D+ReLU forward and MaxPool2D+ReLU backward as one kernel each
// (bit-identical results, every layer's output / delta tensor is still produced); false = one kernel per layer call
extern bool fuse_layers;
// addition (default ON since round 3): inside a container, Conv2D -> ReLU -> MaxPool2D(2,2) blocks run as ONE kernel and their
// backward passes work from the pooled domain; convolutions followed by a ReLU write only the ReLU output where the kernel
// supports it.  The tensors that are not written in such a pass (the block's Conv2D / ReLU outputs, pre-activations) stay
// OBSERVABLE: Layer::get_output() re-computes them on demand -- one forward launch from the recorded input with the parameters
// the last forward pass used (the container keeps a snapshot across its SGD step) -- bit-identical to the unfused pass, so
// the reference's contract (alexnet.cpp:97,105: every layer's output readable after forward) holds.  false = every tensor is
// written by the pass itself.
extern bool fuse_pool_block;
// addition: LinearLayer::forward normally copies its (tiny) output to the host right away, because the reference's callers
// read `output[b]->data` directly (softmax, func.cpp:24-28; argmax, cnn.cpp:92) -- one blocking D2H per forward pass.  While
// this flag is set the copy is skipped (Layer::get_output() / Tensor3D::sync_to_host() still materialise it on demand):
// Sequential::train_step sets it around its forward pass, so a train step never waits for the device.
extern bool lazy_host_sync;
// addition (round 4, default TRUE = the reference's behaviour): Conv2D::backward of the network's FIRST layer computes the delta with
// respect to the input image (conv2d.cpp:168-199) although nothing consumes it (alexnet.cpp:53-55 drops the last backward's return value).
// false: Sequential::train_step does not compute it for a pool-fused first block -- what every training framework does for an input that
// needs no gradient; the layer's delta tensors are then NOT valid after the step (the accessors of the C handle API report that).  Grad-CAM
// and the plain forward / backward / update_gradients sequence are unaffected.  bench.py reports this mode as an extra, labelled leg only.
extern bool input_gradient;

class WithoutGrad final {
public:
    explicit WithoutGrad() { architectures::no_grad = true; }
    ~WithoutGrad() noexcept { architectures::no_grad = false; }
};

// One contiguous NCHW device buffer + the B Tensor3D views over it that the std::vector<tensor> API needs.
class BatchBuffer {
public:
    BatchBuffer() = default;
    BatchBuffer(const BatchBuffer&) = delete;
    BatchBuffer& operator=(const BatchBuffer&) = delete;
    void allocate(int B, int C, int H, int W, const std::string& name);  // (again: the old views are dropped, the memory only grows)
    bool empty() const { return views.empty(); }
    cnn_amd_host::Workspace mem;
    data_type* base = nullptr;  // == mem.ptr
    size_t sample_len = 0;
    std::vector<tensor> views;
};

// returns the device base pointer of a batch: zero-copy when the tensors are consecutive views of one arena,
// otherwise uploads / gathers them into `staging` (host tensors, or views from different arenas)
data_type* batch_device_pointer_mut(const std::vector<tensor>& batch, BatchBuffer& staging, const std::string& who);
inline const data_type* batch_device_pointer(const std::vector<tensor>& batch, BatchBuffer& staging, const std::string& who) {
    return batch_device_pointer_mut(batch, staging, who);
}

class Layer {
public:
    const std::string name;
    std::vector<tensor> output;

public:
    Layer(std::string& _name) : name(std::move(_name)) {}
    virtual ~Layer() = default;
    virtual std::vector<tensor> forward(const std::vector<tensor>& input) = 0;
    virtual std::vector<tensor> backward(std::vector<tensor>& delta) = 0;
    virtual void update_gradients(const data_type learning_rate = 1e-4) {}
    virtual void save_weights(std::ofstream& writer) const {}
    virtual void load_weights(std::ifstream& reader) {}
    // host-readable copy of the last forward's output (alexnet.cpp:97,105 contract): syncs device -> host.  As many tensors as that
    // pass was given (last_B), not the whole buffer's views
    virtual std::vector<tensor> get_output() const;
    // ---- additions: flat parameter arena support (one SGD kernel, one all-reduce per step) ----
    virtual size_t param_count() const { return 0; }
    virtual void bind_arena(data_type* params_dev, data_type* grads_dev) {}
    // addition (Sequential::set_optimizer): the parts of this layer's parameter block that weight decay applies to, as [begin, end)
    // offsets inside the block, ascending.  Default policy: weights only; bias_and_norm extends it to biases and BatchNorm2D's
    // gamma / beta.  BatchNorm2D's moving statistics are never decayed.
    typedef std::vector<std::pair<size_t, size_t> > RangeList;
    virtual void decay_ranges(bool bias_and_norm, RangeList& out) const {}
    // addition (Sequential::set_lamb / set_lars): the tensors inside this layer's parameter block as [begin, end) offsets that tile the
    // whole block, in checkpoint order -- Conv2D / LinearLayer: weights, bias; BatchNorm2D: gamma, beta, moving_mean, moving_var.
    virtual void param_tensors(RangeList& out) const {}
    // ---- additions: what a container tells "whoever cares" (no-ops by default) ----
    // the parameters the last forward pass used are gone (written from outside, or stepped twice without a forward pass in between):
    // an output that pass did not write can no longer be re-computed -- get_output() of it then fails loudly instead of returning a
    // tensor the pass never produced
    virtual void params_of_last_forward_lost() {}
    virtual void set_param_snapshot(const data_type* snap, const bool* active) {}  // see ParamBlock
    virtual void join_pending(void* on_stream) {}   // work of this layer that still runs beside `on_stream` is ordered into it
    virtual void invalidate_prepared() {}           // the parameters changed: copies derived from them are stale
    // data parallelism (Sequential::set_comm): the communicator of the gradient exchange, the one for statistics over the global batch
    virtual void set_comm(void* grads_comm, void* stats_comm, int world, int rank) {}

protected:
    typedef cnn_amd_host::Mark Mark;
    typedef cnn_amd_host::Workspace Workspace;
    typedef cnn_amd_host::ParamBlock ParamBlock;
    // The shape-static contract (conv2d.cpp:47-60): the output buffer is sized by the first forward's batch; later batches may be
    // smaller, never larger, and have the first one's sample shape.
    struct Shape { int C, H, W; };
    Shape in{0, 0, 0};  // sample shape of the first forward's input (0 = not known yet)
    int batch = 0;      // ... and its batch size: the capacity of every buffer
    int last_B = 0;     // batch size of the latest forward pass
    // first call: allocates out_buf [B] x out and sets `output` (returns true).  Every call: B <= batch, `now` == `in` (fatal: abort() with a
    // message naming the layer and both shapes -- a different shape would overrun device memory; otherwise an assert), last_B = B.
    bool static_output(BatchBuffer& out_buf, int B, Shape now, Shape out, bool fatal);
    void require_recomputable(const ParamBlock& pb, const char* what) const;  // throws when pb.lost
};

class ReLU;
class MaxPool2D;
class BatchNorm2D;

class Conv2D : public Layer {
private:
    ReLU* fused_relu = nullptr;  // the ReLU layer right behind this convolution (set by the container), or null
    MaxPool2D* fused_pool = nullptr;  // ... and the MaxPool2D(2,2) behind that ReLU: Conv -> ReLU -> MaxPool in one kernel
    ReLU* relu_below = nullptr;       // the ReLU layer whose output is this layer's input: its backward pass is fused in
    bool publish_backward = false;
    MaxPool2D* pool_below = nullptr;  // the MaxPool2D whose output is this layer's input, when that pool closes a fusable
                                      // Conv2D -> ReLU -> MaxPool2D(2,2) block (fuse_pool_block): see backward()
    Mark pool_fused_pass;             // (backward mark) this pass' forward went through the pooled kernel: backward receives d(pool output)
    void* prep_fwd = nullptr;    // prepared filters (forward / data gradient layouts)
    void* prep_dgrad = nullptr;
    void* prep_dgrad_alt = nullptr;   // second data-gradient image: a DEFERRED data gradient keeps reading the filters of its own step
    // ---- re-materialisation of an output tensor the pass did not write (fuse_pool_block) ----
    mutable bool out_valid = true;    // out_buf holds the last forward's output
    bool delta_valid = true;          // see delta_computed()
    const data_type* last_x = nullptr;  // device pointer of the last forward's input (recorded even under no_grad)
    bool prepared_active = false;
    void* prep_event = nullptr;  // see wait_before_forward
    const int in_channels, out_channels, kernel_size, stride;
    const int params_for_one_kernel;
    const int padding;  // extension: the reference has no padding (conv2d.cpp:41-42 keeps it at 0)
    std::default_random_engine seed;
    // device state: weights [Co][Ci][k][k] then bias [Co], same order as the checkpoint (conv2d.cpp:220-226)
    ParamBlock pb;
    bool grads_ready = false;
    BatchBuffer out_buf, delta_buf, in_stage, delta_stage;
    const data_type* saved_input = nullptr;  // device pointer of the last forward's input (the reference keeps __input)
    std::vector<tensor> saved_input_tensors;  // keeps host-uploaded inputs alive like conv2d.cpp:62
    Workspace workspace;
    void ensure_workspace(int B, int H, int W);
    cnn_conv2d_desc backward_prelude(int B);  // what backward() and backward_weight_pooled() start with: desc, delta buffer, workspace
    // data parallelism (Sequential::set_comm): rank 0 measures the implicit-GEMM tile of this geometry, every replica pins ITS choice
    void* comm = nullptr;
    int comm_world = 1, comm_rank = 0;
    void tune_geometry(const cnn_conv2d_desc& d0);
    data_type* w_dev() const { return pb.params; }
    data_type* b_dev() const { return pb.params + (size_t)out_channels * params_for_one_kernel; }
    data_type* gb_dev() const { return pb.grads + (size_t)out_channels * params_for_one_kernel; }

public:
    // (the trailing _padding argument is an extension for VGG / ResNet-shaped stacks; default = the reference's 0)
    Conv2D(std::string _name, const int _in_channels = 3, const int _out_channels = 16, const int _kernel_size = 3,
           const int _stride = 2, const int _padding = 0);
    ~Conv2D() override;
    std::vector<tensor> forward(const std::vector<tensor>& input) override;
    std::vector<tensor> backward(std::vector<tensor>& delta) override;
    void update_gradients(const data_type learning_rate = 1e-4) override;
    void save_weights(std::ofstream& writer) const override;
    void load_weights(std::ifstream& reader) override;
    int get_params_num() const;
    void set_fused_relu(ReLU* relu) { fused_relu = relu; }  // addition (see architectures::fuse_layers)
    void set_comm(void* grads_comm, void* stats_comm, int world, int rank) override { comm = grads_comm; comm_world = world; comm_rank = rank; }
    void set_fused_pool(MaxPool2D* pool) { fused_pool = pool; }
    void set_relu_below(ReLU* relu) { relu_below = relu; }
    void set_pool_below(MaxPool2D* pool) { pool_below = pool; }
    // addition: the layer that consumes this layer's data gradient next is a convolution (only fused-away layers in between):
    // the data-gradient kernel then publishes its completion (cnn_amd_publish_next_kernel) for that layer's weight-gradient fork
    void set_publish_backward(bool on) { publish_backward = on; }
    // additions: filter re-layout hoisted out of forward / backward (cnn_conv2d_prepare_filters); the container prepares
    // all layers with one call after every parameter change and switches the layers to the *_prepared entry points
    bool shape_known() const { return batch > 0; }
    cnn_conv2d_desc current_desc() const { return cnn_conv2d_desc{batch, in_channels, in.H, in.W, out_channels, kernel_size, stride, padding, 0}; }
    const data_type* filters_dev() const { return pb.params; }
    const data_type* bias_dev() const { return b_dev(); }
    void prepared_buffers(void** fwd, void** dgrad);  // allocated on first use
    void set_prepared(bool on) { prepared_active = on; }
    void invalidate_prepared() override { prepared_active = false; }
    // the prepared images of this layer (and of every later one) are written on another stream: the next forward call waits
    void wait_before_forward(void* event) { prep_event = event; }
    size_t param_count() const override { return (size_t)get_params_num(); }
    void decay_ranges(bool bias_and_norm, RangeList& out) const override {
        out.emplace_back((size_t)0, bias_and_norm ? param_count() : (size_t)out_channels * params_for_one_kernel);
    }
    void param_tensors(RangeList& out) const override {
        const size_t w = (size_t)out_channels * params_for_one_kernel;
        out.emplace_back((size_t)0, w);
        if (param_count() > w) out.emplace_back(w, param_count());
    }
    void bind_arena(data_type* params_dev, data_type* grads_dev) override;
    // ---- additions for fuse_pool_block ----
    // alexnet.cpp:97,105: the output of the last forward, also when that pass fused it away (see architectures::fuse_pool_block)
    std::vector<tensor> get_output() const override;
    void materialize() const;  // writes the missing output tensor(s) of the last forward pass now (no-op when present)
    void set_param_snapshot(const data_type* snap, const bool* active) override { pb.snapshot = snap; pb.snapshot_active = active; }
    void params_of_last_forward_lost() override { pb.lost = true; }
    // The pieces of Conv2D::backward a container schedules itself for the pool-fused FIRST block of a network (nothing consumes
    // that layer's data gradient, conv2d.cpp:168-199 / alexnet.cpp:55):
    struct DeferredDgrad {   // everything the data gradient of one pass needs, valid until that pass' buffers are rewritten
        const void* prepared = nullptr;
        const data_type* dpool = nullptr;
        const int* mask = nullptr;
        const data_type* pooled = nullptr;
        int B = 0;
        int flags = 0;  // cnn_conv2d_desc.flags of the forward call that wrote the mask
        bool valid = false;
    };
    bool pool_fused_pending() const { return pool_fused_pass.armed(); }
    // will forward() of a batch of B samples run the Conv2D -> ReLU -> MaxPool2D(2,2) kernel (the pool then writes the set of
    // buffers a deferred data gradient of the previous pass does NOT read)?  Otherwise the unfused MaxPool2D::forward rewrites set 0.
    bool next_pass_pool_fused(int B) const;
    // cnn_conv2d_desc.flags of the last pool-fused forward pass (CNN_CONV2D_POOL_MASK_PACKED where the library supports it: the
    // block's three kernels then move one byte per pooling window instead of an int32 index -- 111 MB less per step of the reference
    // net); the pass' backward calls must hand the mask back with the same flags
    int pool_mask_flags = 0;
    // weight / bias gradient from the pooled domain on `stream`; with fused_sgd also this layer's SGD step (the old values go to
    // the snapshot) and its filter images for the next pass in the same launch (cnn_conv2d_backward_weight_pooled2_sgd_keep).
    // Returns what the data gradient of this pass will need (launch_deferred_dgrad).
    DeferredDgrad backward_weight_pooled(std::vector<tensor>& delta, bool fused_sgd, data_type learning_rate, data_type grad_scale);
    void prepare_own_filters();  // fwd image + the NEXT data-gradient image from the current parameters, on architectures::stream
    void launch_deferred_dgrad(const DeferredDgrad& job, void* on_stream);
    const data_type* delta_dev() const { return delta_buf.base; }  // the data gradient of the last backward pass (device)
    bool delta_computed() const { return delta_valid; }   // false: the last train_step skipped it (architectures::input_gradient = false)
    void set_delta_computed(bool on) { delta_valid = on; }
    size_t delta_floats() const { return delta_buf.sample_len * delta_buf.views.size(); }
};

// addition: depthwise convolution (one k x k filter per channel, C -> C; the 3x3 half of a depthwise-separable block, the other half
// is Conv2D with a 1x1 kernel).  A desc with CNN_CONV2D_DEPTHWISE through the plain C entry points: no fusion wiring, no prepared
// filters, no tuning -- to a container it is an unfused layer with a parameter block.  Parameters: weights [C][1][k][k] then bias [C],
// initialised by Conv2D's scheme (the layer's own engine, seed 212, bias first, N(0, 1) / random_times).
class DepthwiseConv2D : public Layer {
private:
    const int channels, kernel_size, stride, padding;
    std::default_random_engine seed;
    ParamBlock pb;
    bool grads_ready = false;
    BatchBuffer out_buf, delta_buf, in_stage, delta_stage;
    const data_type* saved_input = nullptr;
    std::vector<tensor> saved_input_tensors;
    Workspace workspace;
    size_t weight_count() const { return (size_t)channels * kernel_size * kernel_size; }
    cnn_conv2d_desc desc(int B) const { return cnn_conv2d_desc{B, channels, in.H, in.W, channels, kernel_size, stride, padding, CNN_CONV2D_DEPTHWISE}; }

public:
    DepthwiseConv2D(std::string _name, const int _channels, const int _kernel_size = 3, const int _stride = 1, const int _padding = 1);
    std::vector<tensor> forward(const std::vector<tensor>& input) override;
    std::vector<tensor> backward(std::vector<tensor>& delta) override;
    void update_gradients(const data_type learning_rate = 1e-4) override;
    void save_weights(std::ofstream& writer) const override;
    void load_weights(std::ifstream& reader) override;
    size_t param_count() const override { return weight_count() + (size_t)channels; }
    void decay_ranges(bool bias_and_norm, RangeList& out) const override { out.emplace_back((size_t)0, bias_and_norm ? param_count() : weight_count()); }
    void param_tensors(RangeList& out) const override {
        out.emplace_back((size_t)0, weight_count());
        out.emplace_back(weight_count(), param_count());
    }
    void bind_arena(data_type* params_dev, data_type* grads_dev) override;
};

class MaxPool2D : public Layer {
private:
    const int kernel_size, step, padding;
    BatchBuffer out_buf, delta_buf, in_stage, delta_stage;
    int* mask = nullptr;  // device int32 [B][C*Ho*Wo], flat indices into the sample's C*H*W (pool2d.cpp:81)
    // a container that DEFERS the data gradient of the block in front (it reads pooled + mask of ITS pass while the next forward
    // pass is already writing new ones) lets the fused forward alternate between two sets
    BatchBuffer out_buf_alt;
    int* mask_alt = nullptr;
    bool alternate = false;
    int cur_set = 0;
    ReLU* fused_relu_below = nullptr;  // the ReLU layer whose output is this pool's input (set by the container), or null
    BatchNorm2D* fused_bn_below = nullptr;  // ... and the BatchNorm2D in front of THAT (BatchNorm2D -> ReLU -> this pool), or null
    Mark forward_done;            // (forward mark) this pass' output + mask were written by the producer's kernel ...
    Mark delta_to_producer;       // (forward mark, armed with forward_done) ... whose backward kernels consume the pooled-domain delta
    Mark backward_passthrough;    // (backward mark, armed by this layer's forward() of such a pass) the delta passes through untouched

public:
    MaxPool2D(std::string _name, const int _kernel_size = 2, const int _step = 2)
        : Layer(_name), kernel_size(_kernel_size), step(_step), padding(0) {}
    ~MaxPool2D() override;
    void set_fused_relu_below(ReLU* relu) { fused_relu_below = relu; }  // addition (see architectures::fuse_layers)
    void set_fused_bn_below(BatchNorm2D* bn) { fused_bn_below = bn; }   // addition: the three layers' backward passes as two kernels
    bool plain_2x2() const { return kernel_size == 2 && step == 2 && padding == 0; }
    // additions used by Conv2D when the container fused Conv2D -> ReLU -> this pool into one kernel
    bool fusable_2x2() const { return kernel_size == 2 && step == 2; }
    // arms forward_done; takes_delta: backward() of this pass hands the delta through to the producer (false: it runs here)
    void fused_forward_target(int B, int C, int H, int W, bool record, bool takes_delta, data_type** pooled, int** mask_out);
    const data_type* pooled_dev() const { return cur_set ? out_buf_alt.base : out_buf.base; }
    const int* mask_dev() const { return cur_set ? mask_alt : mask; }
    void enable_alternate_sets() { alternate = true; }
    // pool-fused pass: the delta of this pool's output passes through untouched (the block's Conv2D consumes it).  The block's
    // ReLU::backward -- in the pooled domain: d(pool_out) masked by (pool_out <= 0), because at an argmax position the ReLU
    // output equals the pooled value and everywhere else the delta is 0 either way -- is carried by the mask itself: the fused
    // forward kernel sets bit 31 of a window's mask entry when its pooled value is <= 0, and the pooled-domain gradient kernels
    // then never match that window.
    void fused_forward_none() { forward_done.clear(); delta_to_producer.clear(); }  // the producer says that this pass' forward() runs here
    bool passthrough_armed() const { return backward_passthrough.armed(); }
    std::vector<tensor> forward(const std::vector<tensor>& input) override;
    std::vector<tensor> backward(std::vector<tensor>& delta) override;
};

class ReLU : public Layer {
private:
    BatchBuffer out_buf, in_stage, delta_stage;
    Mark forward_done;           // (forward mark) this pass' output was already written by the producing Conv2D / BatchNorm2D kernel
    Mark backward_done;          // (backward mark) this pass' delta was already masked by the consuming layer's kernel
    bool out_valid = true;       // false: the pool-fused pass did not write this layer's output (get_output re-computes it)
    const Conv2D* producer = nullptr;  // the convolution whose kernel writes this layer's output when fused
    const BatchNorm2D* bn_producer = nullptr;  // ... or the normalisation (BatchNorm2D -> ReLU -> MaxPool2D in one apply pass)

public:
    ReLU(std::string _name) : Layer(_name) {}
    std::vector<tensor> get_output() const override;
    bool output_valid() const { return out_valid; }
    void set_producer(const Conv2D* conv) { producer = conv; }
    void set_bn_producer(const BatchNorm2D* bn) { bn_producer = bn; }
    data_type* rematerialize_target() const { const_cast<ReLU*>(this)->out_valid = true; return out_buf.base; }
    // additions used by Conv2D / MaxPool2D when the container fused this layer into their kernels
    data_type* fused_forward_target(int B, int C, int H, int W);  // output arena (allocated on first use); arms forward_done
    void fused_forward_none() { forward_done.clear(); }        // ... or says that this pass' forward() runs here
    void fused_backward(bool done) { backward_done.set(done); }  // the consumer's backward states whether it masked the delta
    void fused_forward_skipped(int B, int C, int H, int W);  // pool-fused pass: the output is never materialised
    std::vector<tensor> forward(const std::vector<tensor>& input) override;
    std::vector<tensor> backward(std::vector<tensor>& delta) override;
};

class LinearLayer : public Layer {
private:
    const int in_channels, out_channels;
    ParamBlock pb;  // W [in][out] then bias [out] (linear.cpp:105-108)
    bool grads_ready = false;
    std::tuple<int, int, int> delta_shape;
    BatchBuffer out_buf, delta_buf, in_stage, delta_stage;
    const data_type* saved_input = nullptr;
    std::vector<tensor> saved_input_tensors;
    ReLU* relu_below = nullptr;  // the ReLU layer whose output is this layer's input: its backward pass is fused in
    bool publish_backward = false;
    Mark head_dx_done;           // (backward mark) this pass' data gradient was written by the loss-head kernel (forward_loss_head(with_dx))
    void* ev_head = nullptr;
    void* own_stream = nullptr;  // the weight / bias gradient of such a pass runs here, beside everything else ...
    void* ev_wb = nullptr;
    bool wb_pending = false;     // ... until join_pending() orders it into a stream

public:
    void set_relu_below(ReLU* relu) { relu_below = relu; }  // addition (see architectures::fuse_layers)
    void set_publish_backward(bool on) { publish_backward = on; }  // (see Conv2D::set_publish_backward)
    // the weight / bias gradient of a loss-head pass may still be running on the layer's own stream: `on_stream` waits for it
    // (containers call this before they read the gradient arena; update_gradients() of a stand-alone layer does it itself)
    void join_pending(void* on_stream) override;
    // addition: forward + softmax + cross-entropy delta in ONE kernel (cnn_linear_forward_softmax_xent, out_channels <= 8):
    // labels_dev int32 [B]; delta_dev [B][out] receives p - onehot (func.cpp:56-73), loss_terms_dev [B] log p[label]
    bool loss_head_supported() const { return out_channels <= 8; }
    // with_dx: the same kernel also writes this layer's data gradient (cnn_linear_forward_softmax_xent_dx: a sample's row needs only
    // that sample's delta); backward() then only launches the weight / bias gradient, on the library's side stream
    // targets_dev != nullptr: dense targets, float [B][out] on the device, take the labels' place (labels_dev is not read): the
    // cnn_linear_forward_softmax_xent_soft* entries, delta = p - target, loss term sum_j log p[j] * target[j]
    std::vector<tensor> forward_loss_head(const std::vector<tensor>& input, const int* labels_dev, data_type* probs_dev,
                                          data_type* delta_dev, data_type* loss_terms_dev, bool with_dx = false,
                                          const data_type* targets_dev = nullptr);
    int out_features() const { return out_channels; }
    int in_features() const { return in_channels; }
    LinearLayer(std::string _name, const int _in_channels, const int _out_channels);
    ~LinearLayer() override;
    std::vector<tensor> forward(const std::vector<tensor>& input) override;
    std::vector<tensor> backward(std::vector<tensor>& delta) override;
    void update_gradients(const data_type learning_rate = 1e-4) override;
    void save_weights(std::ofstream& writer) const override;
    void load_weights(std::ifstream& reader) override;
    size_t param_count() const override { return (size_t)in_channels * out_channels + out_channels; }
    void decay_ranges(bool bias_and_norm, RangeList& out) const override {
        out.emplace_back((size_t)0, bias_and_norm ? param_count() : (size_t)in_channels * out_channels);
    }
    void param_tensors(RangeList& out) const override {
        out.emplace_back((size_t)0, (size_t)in_channels * out_channels);
        out.emplace_back((size_t)in_channels * out_channels, param_count());
    }
    void bind_arena(data_type* params_dev, data_type* grads_dev) override;
};

// architectures.h:143-173 / batchnorm2d.cpp.  Device state: gamma [C], beta [C], moving_mean [C], moving_var [C] in ONE
// block in checkpoint order (batchnorm2d.cpp:168-173); the gradient block has the same shape, its moving_* half stays 0
// so that the flat-arena SGD kernel leaves the statistics untouched.  The reference's normed_input buffer is not kept
// (backward recomputes it from the recorded input and the saved batch statistics).
class BatchNorm2D : public Layer {
private:
    const int out_channels;
    const data_type eps;
    const data_type momentum;
    ParamBlock pb;
    bool grads_ready = false;
    Mark backward_done_by_pool;  // (backward mark) this pass' backward() already ran inside the pool's (see backward_pooled)
    data_type* saved_stats = nullptr;  // batch mean [C] then batch variance [C] (buffer_mean / buffer_var)
    BatchBuffer out_buf, in_stage, delta_stage;
    const data_type* saved_input = nullptr;
    std::vector<tensor> saved_input_tensors;
    Workspace workspace;
    void* comm = nullptr;        // RCCL communicator: statistics over the GLOBAL batch (sync-BN), see Sequential::set_comm
    int comm_world = 1;
    data_type* sync_sums = nullptr;  // [C] + [C] + [C][4] all-reduce operands
    ReLU* fused_relu = nullptr;      // the ReLU layer right behind this one (set by the container): its output comes from the apply pass
    MaxPool2D* fused_pool = nullptr; // ... and the MaxPool2D behind THAT: pooled in the same pass
    // ---- fuse_pool_block: a training pass with a fused ReLU behind this layer writes ONLY the ReLU output (round 4); get_output() of
    // this layer re-computes the normalised tensor from the recorded input, the saved batch statistics and the gamma / beta of that pass
    mutable bool out_valid = true;

public:
    void set_comm(void* grads_comm, void* stats_comm, int world, int rank) override { comm = stats_comm; comm_world = world; }
    void set_fused_relu(ReLU* relu) { fused_relu = relu; }
    void set_fused_pool(MaxPool2D* pool) { fused_pool = pool; }  // addition: BatchNorm2D -> ReLU -> MaxPool2D(2, 2) in one apply pass
    void materialize_relu() const;  // the ReLU output of a pass that wrote only the pooled tensor (ReLU::get_output)
    // additions used by the MaxPool2D behind this layer's ReLU (BatchNorm2D -> ReLU -> MaxPool2D(2, 2)): its backward pass runs this
    // layer's from the pooled domain (cnn_batchnorm2d_backward_pooled: bit-identical) and arms the pass-through of backward()
    bool backward_pooled_possible(int B) const;
    void backward_pooled(const data_type* dpool, const int* mask, const data_type* pooled, data_type* dx, int B);
    void backward_not_pooled() { backward_done_by_pool.clear(); }  // the pool's backward of this pass did not take that path
    std::vector<tensor> get_output() const override;
    void materialize() const;
    void set_param_snapshot(const data_type* snap, const bool* active) override { pb.snapshot = snap; pb.snapshot_active = active; }
    void params_of_last_forward_lost() override { pb.lost = true; }
    BatchNorm2D(std::string _name, const int _out_channels, const data_type _eps = 1e-5, const data_type _momentum = 0.1);
    ~BatchNorm2D() override;
    std::vector<tensor> forward(const std::vector<tensor>& input) override;
    std::vector<tensor> backward(std::vector<tensor>& delta) override;
    void update_gradients(const data_type learning_rate = 1e-4) override;
    void save_weights(std::ofstream& writer) const override;
    void load_weights(std::ifstream& reader) override;
    size_t param_count() const override { return (size_t)4 * out_channels; }
    void decay_ranges(bool bias_and_norm, RangeList& out) const override {  // gamma, beta -- never moving_mean / moving_var
        if (bias_and_norm) out.emplace_back((size_t)0, (size_t)2 * out_channels);
    }
    void param_tensors(RangeList& out) const override {
        for (size_t k = 0; k < 4; ++k) out.emplace_back(k * out_channels, (k + 1) * out_channels);
    }
    void bind_arena(data_type* params_dev, data_type* grads_dev) override;
};

// architectures.h:177-191 / dropout.cpp: CHANNEL dropout.  The reference keeps it out of its network (alexnet.cpp:28, "poor at
// test time", README.md:16) but ships the layer; same constructor, generator (seed 1314) and bookkeeping.  Training zeroes the
// first int(p * C) channels of every sample (dropout.cpp:34-41 tests the channel index, the shuffled sequence only fills the
// mask), no_grad scales by 1 - p; backward zeroes the same channels of the delta in place and hands it back.
class Dropout : public Layer {
private:
    data_type p;
    int selected_num = 0;
    std::vector<int> sequence;
    std::default_random_engine drop;
    std::vector<int> mask;
    BatchBuffer out_buf, in_stage, delta_stage;

public:
    Dropout(std::string _name, const data_type _p = 0.5) : Layer(_name), p(_p), drop(1314) {}
    std::vector<tensor> forward(const std::vector<tensor>& input) override;
    std::vector<tensor> backward(std::vector<tensor>& delta) override;
};

// what Sequential::eval_result returns: cnn_eval_result's totals and the two figures a caller derives from them
struct EvalResult {
    uint64_t samples = 0, top1 = 0, topk = 0, ignored = 0;
    double loss_sum = 0;
    double mean_loss() const { return loss_sum / (double)samples; }
    double accuracy() const { return (double)top1 / (double)samples; }
};

// The reference's model container is a strictly sequential std::list<std::shared_ptr<Layer>> (architectures.h:200) that
// forward walks front to back (alexnet.cpp:41-42), backward back to front (:53-55), update / save / load front to back
// (:63-64, :73-74, :86-87).  Sequential is that container for ANY layer list (the reference hard-wires one list in
// AlexNet's constructor); AlexNet below is the reference's list on top of it.  Additions over the reference's container:
//   * one flat parameter / gradient arena in checkpoint order (= layer order), so the SGD step is one kernel, a .model
//     file one copy and the data-parallel exchange one (or a few bucketed) all-reduce(s);
//   * fusion wiring between neighbouring layers (architectures::fuse_layers / fuse_pool_block);
//   * filter preparation hoisted out of the per-layer calls (cnn_conv2d_prepare_filters), redone after every parameter change;
//   * an optional RCCL communicator (set_comm): the batch is then sharded over `world` replicas, BatchNorm2D layers
//     normalise over the GLOBAL batch (sync-BN) and update_gradients() sums the gradient arena over the replicas first;
//   * an optional optimizer on the arena instead of the reference's w -= lr * g -- one of momentum SGD (set_optimizer), Adam / AdamW
//     (set_adam), LAMB (set_lamb), LARS (set_lars); the setter called last is the active kind (OptKind, optimizer.cpp);
//   * clipping by the global gradient norm (set_grad_clip) in front of whichever step is active;
//   * gradient accumulation over micro-batches (set_grad_accumulation): k container steps, one optimizer step on their summed gradients;
//   * an exponential moving average of the parameters (set_ema) behind every optimizer step, swapped into the arena for evaluation
//     and export (swap_ema), with a state file of its own (save_ema_state / load_ema_state);
//   * evaluation on the device (eval_begin / eval_step / eval_result): loss, top-1 / top-k and confusion counts, one read-back at the end.
class Sequential {
public:
    bool print_info = false;

protected:
    std::list<std::shared_ptr<Layer> > layers_sequence;
    data_type* param_arena = nullptr;  // every layer's parameters in checkpoint order
    data_type* grad_arena = nullptr;
    size_t n_params = 0;
    bool owns_arena = false;
    bool finalized = false;
    bool filters_prepared = false;  // the layers' prepared filters match the current parameters
    void* comm = nullptr;           // RCCL communicator (cnn_comm_*), not owned
    int comm_world = 1;
    void* bn_comm = nullptr;        // a second communicator over the same ranks for BatchNorm2D's sync-BN reductions (owned; cnn_comm_split)
    void* comm_stream = nullptr;    // the exchange runs on its own stream, gated by events
    void* ev_grads = nullptr;
    void* ev_prep = nullptr;   // filter images of layers 2.. prepared on the library's side stream (prepare_filters)
    void* ev_prep_fork = nullptr;
    void* ev_comm = nullptr;
    bool grads_reduced = false;     // this step's gradient arena has been summed over the replicas
    std::vector<size_t> layer_offsets;  // arena offset of every layer's parameter block (finalize)
    // ---- fuse_pool_block support (round 3) ----
    data_type* param_prev = nullptr;  // the parameters as they were before the latest SGD step (Conv2D::materialize)
    bool params_stepped = false;      // ... which happened after the last forward pass
    // the pool-fused FIRST block of the network (Conv2D -> ReLU -> MaxPool2D(2,2) at the front), if there is one: train_step
    // defers its data gradient into the next forward pass and runs the rest of the step's tail underneath its weight gradient
    Conv2D* block_conv = nullptr;
    MaxPool2D* block_pool = nullptr;
    Layer* behind_block = nullptr;     // the layer that consumes the pool's output (its backward rewrites d(pool output))
    Layer* release_after = nullptr;    // the deferred data gradient starts behind this layer's forward kernel
    void* defer_stream = nullptr;
    void* ev_defer_done = nullptr;
    void* ev_tail = nullptr;
    void* ev_side_tail = nullptr;
    bool side_tail_pending = false;  // the side stream still runs the previous step's tail (fused_tail, TAIL_BEHIND_BLOCK)
    void prepare_later_filters(void* on_stream);
    Conv2D::DeferredDgrad pending_dgrad;
    bool defer_in_flight = false;
    bool fused_tail(std::vector<tensor>& delta, const data_type learning_rate);  // false: not applicable to this pass
    // big arenas (the VGG / ResNet-shaped stacks: 37 - 45 MB) are exchanged in BUCKETS while the backward pass is still running:
    // layers are walked back to front, so finished gradients form a growing suffix of the arena; every >= bucket_floats of it
    // go out on the communication stream behind an event.  Small arenas (the reference net: 445 KB, latency-bound) stay one call.
    size_t bucket_floats = (size_t)2 << 20;
    void flush_bucket(size_t lo, size_t hi);
    // ---- the optimizer (optimizer.cpp): ONE kind says which step the container takes on its arena; each kind has its options, and
    // all of them share one block of state.  set_optimizer / set_adam / set_lamb / set_lars replace each other by assigning the kind.
    enum class OptKind {
        kPlain,  // the reference's w -= lr * g (cnn_sgd_update_keep): every launch as without an optimizer
        kSgdm,   // cnn_sgd_momentum_update on arena ranges
        kAdam,   // cnn_adam_update on arena ranges
        kLamb,   // ONE cnn_lamb_update over the whole arena
        kLars,   // ONE cnn_lars_update over the whole arena
    };
    OptKind opt_kind = OptKind::kPlain;
    // what the call sites ask of the kind:
    // the step is more than the front block's in-kernel plain SGD -- the fused tail steps that block with the arena kernel, no TAIL_BEHIND_BLOCK
    bool step_beyond_plain_sgd() const { return opt_kind != OptKind::kPlain; }
    // a trust ratio needs every gradient of a tensor before that tensor moves: one call over the whole arena, never range steps
    bool step_needs_whole_tensors() const { return opt_kind == OptKind::kLamb || opt_kind == OptKind::kLars; }
    // the step reads and writes exp_avg / exp_avg_sq and carries the step counter
    bool step_uses_adam_moments() const { return opt_kind == OptKind::kAdam || opt_kind == OptKind::kLamb; }
    // the options of each kind as the setter left them: the C ABI's options struct (lr -- and step -- are filled in per step) plus
    // the policy bits that shape the kind's table.  A kind's options survive while another kind is active.
    struct SgdmOptions {
        cnn_sgd_options abi = {0, 0, 0, 0};
        bool decay_bias_and_norm = false;
    } sgdm_opt;  // (also what a kPlain net's state file carries: momentum 0, weight decay 0)
    struct AdamOptions {
        cnn_adam_options abi = {0, 0, 0, 0, 0, 0, 0};  // (abi.decoupled: Adam's L2 term or AdamW)
        bool decay_bias_and_norm = false;
    } adam_opt;
    struct LambOptions {
        cnn_lamb_options abi = {0, 0, 0, 0, 0, 0};
        bool decay_bias_and_norm = false, adapt_bias_and_norm = false;
    } lamb_opt;
    struct LarsOptions {
        cnn_lars_options abi = {0, 0, 0, 0, 0, 0};
        bool decay_bias_and_norm = false, adapt_bias_and_norm = false;
    } lars_opt;
    struct DecayTable {                // the decayed index ranges inside arena[lo, hi), relative to lo (begin, end pairs)
        size_t lo = 0, hi = 0;
        std::vector<uint32_t> host;
        uint32_t* dev = nullptr;       // device copy, only for tables of more than CNN_SGD_INLINE_RANGES ranges
    };
    // Every arena is n_params floats, allocated and zeroed by the first setter that needs it, never freed or zeroed by a switch.
    struct OptState {
        data_type* velocity = nullptr;                 // kSgdm, kLars (and allocated by set_optimizer(0, 0))
        data_type* exp_avg = nullptr;                  // kAdam, kLamb
        data_type* exp_avg_sq = nullptr;               // kAdam, kLamb
        uint64_t step = 0;                             // kAdam, kLamb: container steps taken under either (the next launch carries step after its increment)
        data_type* lamb_update = nullptr;              // kLamb: scratch, r between its two passes
        // kSgdm, kAdam: the three ranges the container steps -- the whole arena, behind the front block, the front block; rebuilt by
        // set_optimizer / set_adam, left alone by set_lamb / set_lars
        DecayTable decay_tables[3];
        void* layerwise = nullptr;                     // kLamb, kLars: cnn_layerwise_create -- the device table, the norm workspace, the statistics
        std::vector<uint32_t> seg_bounds, seg_flags;   // ... and the segment table it was created from (host copy)
    } opt;
    // what every setter starts with: finalized and the 32-bit table limit (deliberately checked in every build, not asserts: they abort
    // with the setter's name), flush_deferred, synchronize.  (set_grad_accumulation builds no table: its kernel's indices are 64-bit)
    void begin_optimizer_switch(const char* setter, bool builds_32bit_table = true);
    const DecayTable& decay_table_of(size_t lo, size_t hi) const;  // the table built for exactly this range; aborts when there is none
    void ensure_state_arena(data_type*& arena);
    void build_decay_table(DecayTable& t, size_t lo, size_t hi, bool bias_and_norm);
    void build_decay_tables(bool bias_and_norm);
    void build_segment_table(bool decay_bias_and_norm, bool adapt_bias_and_norm);
    struct StateFormat;                               // one on-disk format of the optimizer state (optimizer.cpp)
    // ---- clipping by the global gradient norm (set_grad_clip): orthogonal to the kind ----
    data_type clip_max_norm = 0;       // 0: off
    void* clip_workspace = nullptr;    // cnn_clip_grad_norm's partial sums
    size_t clip_workspace_bytes = 0;
    data_type* clip_stats = nullptr;   // [2] on the device: total norm, coefficient of the latest clipped step
    size_t front_block_params() const;
    // ---- gradient accumulation over micro-batches (set_grad_accumulation): orthogonal to the kind and to clipping ----
    int accum_k = 1;                   // micro-batches per window; 1: off
    int accum_phase = 0;               // micro-batches in the open window, 0 .. accum_k - 1
    data_type* accum_grads = nullptr;  // n_params floats, owned by the container whoever owns the arenas
    // the gradients the exchange, the clip and the step read: the ONE place that decides between the arena and the accumulator
    data_type* step_grads() const { return accum_k > 1 ? accum_grads : grad_arena; }
    // accum_k > 1: counts this container step as one micro-batch -- flush_deferred, ONE cnn_grad_accumulate on the compute stream.
    // true: the call closes the window (the exchange over the accumulator has run, the caller clips and steps); false: it returns
    bool count_micro_batch();
    void exchange_grads(data_type* grads);  // the event-fenced all-reduce of n_params gradients on the communication stream
    // the tail of every container step: [the clip,] the active kind's step over the whole arena reading step_grads(), the snapshot,
    // [the average]
    void clip_and_step(data_type learning_rate, data_type grad_scale);
    // ---- exponential moving average of the parameters (set_ema): orthogonal to the kind, to clipping and to accumulation ----
    struct EmaState {
        data_type decay = 0;               // 0: off (the shadow and the counter are kept)
        bool warmup = false, average_stats = false;
        data_type* shadow = nullptr;       // n_params floats, owned by the container whoever owns the arenas
        uint64_t updates = 0;              // updates taken since the shadow was last (re)filled
        bool swapped = false;              // the arena holds the average, the shadow the training weights (swap_ema)
        DecayTable table;                  // the averaged index ranges of the arena (lo = 0, hi = n_params)
    } ema;
    void build_ema_table(bool average_stats);
    void fill_ema_shadow();                // shadow = parameters (one cnn_ema_update with decay 0), counter = 0
    void unswap_ema() { if (ema.swapped) swap_ema(); }  // what every entry that steps, or touches the average, starts with
    // the step of the active kind on arena[lo, hi) (parameters, gradients, state, snapshot) on `on_stream`: the ONE dispatch on opt_kind.
    // kSgdm / kAdam step the three ranges decay tables exist for; kLamb / kLars the whole arena only.
    void step_arena(size_t lo, size_t hi, data_type learning_rate, data_type grad_scale, void* on_stream);
    bool exchange_active() const;
    void wire();
    void bind(data_type* p, data_type* g);
    void prepare_filters();

public:
    Sequential() = default;
    virtual ~Sequential();
    Sequential(const Sequential&) = delete;
    Sequential& operator=(const Sequential&) = delete;
    // append a layer (takes ownership); all add() calls come before finalize()
    Sequential& add(Layer* layer);
    // wires the fusions and moves every layer's parameters into ONE arena (owned, or caller-provided device buffers of
    // num_params() floats each, e.g. so that a framework can own / all-reduce them)
    void finalize();
    void finalize(data_type* params_dev, data_type* grads_dev);
    std::vector<tensor> forward(const std::vector<tensor>& input);
    void backward(std::vector<tensor>& delta_start);
    void update_gradients(const data_type learning_rate = 1e-4);
    // one SGD kernel over the flat arena; grad_scale folds the 1/G of a data-parallel all-reduce(sum) done by the caller
    void update_gradients(const data_type learning_rate, const data_type grad_scale);
    void save_weights(const std::filesystem::path& save_path) const;
    void load_weights(const std::filesystem::path& checkpoint_path);
    // alexnet.cpp:95-142 (cv::Mat -> the H*W 8-bit pixels of that matrix, row-major; see cnn_grad_cam).  Like the reference it
    // assumes a forward pass with gradients enabled has just run, walks backward() down to the named layer and reads that
    // layer's get_output(); `cam_out` (optional) receives the normalised [B][H][W] map the picture is taken from.
    std::vector<uchar> grad_cam(const std::string& layer_name, std::vector<data_type>* cam_out = nullptr) const;
    // additions
    size_t num_params() const;
    data_type* params_device() const { return param_arena; }
    data_type* grads_device() const { return grad_arena; }
    // MUST be called after writing the parameter arena from outside (memcpy, collective, ...): the convolutions keep
    // re-arranged copies of their filters between update_gradients() calls
    void parameters_changed();
    const std::list<std::shared_ptr<Layer> >& layers() const { return layers_sequence; }
    // SGD with momentum, weight decay and Nesterov for every step the container takes on its arena (update_gradients, train_step):
    // v = momentum * v + (g + weight_decay * w);  w -= lr * (nesterov ? g + weight_decay * w + momentum * v : v) -- torch.optim.SGD's
    // update, formula and rounding in include/cnn_amd.h (cnn_sgd_momentum_update).  Weight decay applies to Conv2D / LinearLayer
    // weights; decay_bias_and_norm extends it to biases and BatchNorm2D's gamma / beta (never to the moving statistics).  Call it
    // after finalize(), any number of times: the velocity arena is allocated and zeroed by the first call and kept by later ones.
    // set_optimizer(0, 0) returns to the reference's plain step.  A train step with an optimizer set steps the front block's
    // parameters with the arena kernel instead of inside its weight-gradient kernel.  Stand-alone
    // Layer::update_gradients(lr) stays the plain step.  Under set_comm the velocity is per replica and needs no exchange.
    void set_optimizer(data_type momentum, data_type weight_decay, bool nesterov = false, bool decay_bias_and_norm = false);
    bool optimizer_active() const { return step_beyond_plain_sgd(); }
    data_type* velocity_device() const { return opt.velocity; }  // null before the first set_optimizer()
    // Optimizer state beside a .model checkpoint (whose format stays the reference's).  One format per optimizer -- a header of magic,
    // n_params, [step,] the setter's options, then the kind's state arenas; each is described once, in optimizer.cpp's format table.
    // save writes the active kind's format (the plain step: the momentum format with momentum 0, weight decay 0); load recognises all
    // of them and activates the optimizer the file was written for.  Both return 0 on success.  save: 1 = cannot write, 4 = no
    // optimizer was ever set.  load: 1 = cannot open, 2 = not such a file / truncated / options out of range, 3 = written for another
    // n_params; nothing is changed on failure, on success the file's options are set as by the setter, then its arenas and step counter.
    // An open accumulation window (set_grad_accumulation) is NOT part of the file -- neither the accumulator nor the phase nor k:
    // save at a window boundary (accumulation_phase() == 0), or the micro-batches of the open window are to be run again after a load.
    int save_optimizer_state(const std::filesystem::path& path);
    int load_optimizer_state(const std::filesystem::path& path);

    // Adam / AdamW (torch.optim.Adam / AdamW, amsgrad off) for every step the container takes on its arena; formula and rounding in
    // include/cnn_amd.h (cnn_adam_update).  decoupled = false adds weight_decay * w to the gradient (Adam's L2 term), true shrinks the
    // parameter by 1 - lr * weight_decay (AdamW); the decay policy is set_optimizer's.  Call it after finalize(), any number of times:
    // the two state arenas (exp_avg, exp_avg_sq) are allocated and zeroed, and the step counter set to 0, by the first call only.
    // set_adam and set_optimizer replace each other -- the one called last is the active optimizer, set_optimizer(0, 0) still returns
    // to the plain step -- and no state arena is freed or zeroed by a switch.  The step counter advances once per container step
    // (update_gradients / train_step), also where the fused tail steps the arena in two launches.  The price in a train step is
    // the momentum optimizer's: the front block is stepped by the arena kernel.
    void set_adam(data_type beta1 = 0.9, data_type beta2 = 0.999, data_type eps = 1e-8, data_type weight_decay = 0, bool decoupled = false,
                  bool decay_bias_and_norm = false);
    bool adam_is_active() const { return opt_kind == OptKind::kAdam; }
    data_type* adam_m_device() const { return opt.exp_avg; }  // null before the first set_adam()
    data_type* adam_v_device() const { return opt.exp_avg_sq; }
    uint64_t adam_step() const { return opt.step; }
    // Clipping by the global L2 norm of the gradient arena (torch.nn.utils.clip_grad_norm_; cnn_clip_grad_norm): with max_norm > 0
    // update_gradients(lr, grad_scale) clips the whole arena -- behind the data-parallel all-reduce, in front of the step, on the same
    // stream, without a host round trip -- for the plain step, the momentum optimizer and Adam alike.  0 (the default) switches it
    // off.  BatchNorm2D's moving statistics have a zero gradient and add nothing to the norm.  THE PRICE: the norm needs every
    // gradient of the step before any parameter moves, so with clipping on the fused step tail (fused_tail) declines and a train
    // step takes the plain sequence -- the whole backward walk, the joins, update_gradients -- plus the three clip launches.
    void set_grad_clip(data_type max_norm);
    data_type grad_clip() const { return clip_max_norm; }
    bool grad_clip_ever_on() const { return clip_stats != nullptr; }
    // total norm (and coefficient) of the latest clipped step; like last_loss() it synchronises.  Asserts when clipping was never on.
    data_type last_grad_norm(data_type* coef_out = nullptr);

    // Layer-wise adaptive rates (include/cnn_amd.h: cnn_lamb_update, cnn_lars_update): LAMB is Adam with a trust ratio per parameter
    // tensor, LARS momentum SGD with one.  The tensors are the layers' param_tensors() at their arena offsets.  CNN_SEG_DECAY follows
    // set_optimizer's decay policy (decay_bias_and_norm); CNN_SEG_ADAPT is set on Conv2D / LinearLayer weights, with
    // adapt_bias_and_norm on biases and BatchNorm2D's gamma / beta as well; the moving statistics never get either flag.  Call them
    // after finalize(), any number of times.  LAMB uses Adam's state (exp_avg, exp_avg_sq, the step counter: allocated and zeroed by
    // whichever of set_adam / set_lamb comes first, never zeroed by a switch), LARS uses the velocity arena.  set_optimizer, set_adam,
    // set_lamb and set_lars replace each other -- the one called last is active, set_optimizer(0, 0) still returns to the plain step.
    // THE PRICE: a trust ratio needs every gradient of a tensor before that tensor moves, so the step is one call over the whole
    // arena inside update_gradients(lr, grad_scale) -- behind the all-reduce and the clip -- and the fused step tail (fused_tail)
    // declines, as under clipping.  Under set_comm the state is per replica and nothing new is exchanged.
    void set_lamb(data_type beta1 = 0.9, data_type beta2 = 0.999, data_type eps = 1e-6, data_type weight_decay = 0, bool decay_bias_and_norm = false,
                  bool adapt_bias_and_norm = false);
    void set_lars(data_type momentum, data_type weight_decay, data_type trust_coefficient = 1e-3, data_type eps = 1e-8, bool nesterov = false,
                  bool decay_bias_and_norm = false, bool adapt_bias_and_norm = false);
    bool layerwise_active() const { return step_needs_whole_tensors(); }
    bool lamb_is_active() const { return opt_kind == OptKind::kLamb; }
    bool lars_is_active() const { return opt_kind == OptKind::kLars; }
    size_t segment_count() const { return opt.seg_flags.size(); }  // 0 before the first set_lamb() / set_lars()
    void segment_table(std::vector<uint32_t>& bounds, std::vector<uint32_t>& flags) const {
        bounds = opt.seg_bounds;
        flags = opt.seg_flags;
    }
    // w_norm, u_norm, ratio of the latest layer-wise step (segment_count() values each); like last_grad_norm() it synchronises.
    // false: no layer-wise optimizer was ever set.
    bool trust_stats(std::vector<data_type>& w_norm, std::vector<data_type>& u_norm, std::vector<data_type>& ratio);

    // Gradient accumulation: a window of micro_steps micro-batches counts as ONE optimizer step on their summed gradients -- the large
    // batch activation memory does not allow.  micro_steps >= 1; 1 (the default) switches it off.  Call it after finalize(), any number
    // of times: the first micro_steps > 1 allocates the accumulator (num_params() floats, owned by the container also where the caller
    // provided the arenas, kept until the container goes).  Calling it with a window open discards that window.
    // With micro_steps = k > 1 every container step -- update_gradients(lr), update_gradients(lr, grad_scale), train_step -- counts one
    // micro-batch: flush_deferred(), then one cnn_grad_accumulate of the gradient arena into the accumulator (a copy of the bits when
    // it opens the window, one fp32 add per element afterwards).  Calls 1 .. k-1 return there: no parameter, optimizer state or step
    // counter moves, lr is ignored, get_output() stays valid; only BatchNorm2D's moving statistics move, with every forward pass as
    // always.  Call k closes the window: the exchange when a communicator is set (ONE all-reduce over the accumulator; the bucketed
    // exchange inside backward() is off and allreduce_gradients() a no-op while k > 1), the clip when it is on, then the active
    // kind's step -- all three read the accumulator.  Its gradient scale is 1 / (k * world) in the one-argument form and
    // grad_scale / k in the two-argument form; the Adam / LAMB step counter advances once per window and last_grad_norm() reports the
    // accumulated gradient's norm.  THE PRICE: the front block's in-kernel SGD step would move parameters in the middle of a window,
    // so the fused step tail (fused_tail) declines while k > 1, as under clipping, and every micro-batch adds one streaming pass over
    // the arena.  With k = 1 nothing changes, not one launch.  The state files do not carry an open window (see below).  Stand-alone
    // Layer::update_gradients and a non-finalized list never accumulate.
    void set_grad_accumulation(int micro_steps);
    int grad_accumulation() const { return accum_k; }
    int accumulation_phase() const { return accum_phase; }                 // micro-batches in the open window, 0 .. k-1
    data_type* accumulated_grads_device() const { return accum_grads; }    // null before the first micro_steps > 1

    // Exponential moving average of the parameters: a shadow copy of the arena that follows every optimizer step,
    //     shadow = d * shadow + (1 - d) * parameters,   d = cnn_ema_decay_at(decay, warmup, updates taken so far)
    // (formula and rounding in include/cnn_amd.h, cnn_ema_update; warmup: d = min(decay, (1 + t) / (10 + t)), 0.1 at first).
    // Call it after finalize(), any number of times.  decay in (0, 1) switches it on, decay == 0 off: the shadow and the counter are
    // kept and nothing more is launched.  The first call with decay > 0 allocates the shadow (num_params() floats, owned by the
    // container also where the caller provided the arenas, kept until the container goes), fills it with a copy of the bits of the
    // current parameters and sets the update counter to 0; later calls change the options only.  Averaged are the layers'
    // decay_ranges(true, ...): weights, biases, BatchNorm2D's gamma / beta.  BatchNorm2D's moving statistics are averages already:
    // the shadow takes their bits as they are, unless average_stats asks for the whole arena.
    // The update is the last launch of every optimizer step (update_gradients(lr), update_gradients(lr, grad_scale), train_step), on
    // the same stream behind the step: ONE cnn_ema_update, 12 bytes per parameter -- once per window under
    // set_grad_accumulation(k > 1).  Under set_comm nothing is exchanged: every replica averages the same parameters.  THE PRICE:
    // the average must follow the WHOLE step, and the fused step tail (fused_tail) finishes the arena on two streams, so it declines
    // while the average is on, as under clipping, trust ratios and accumulation.  With set_ema never called, or off again, nothing
    // changes, not one launch.  Stand-alone Layer::update_gradients and a non-finalized list never average.
    void set_ema(data_type decay, bool warmup = false, bool average_stats = false);
    // shadow = the current parameters (a copy of the bits), counter = 0 -- e.g. after load_weights.  Nothing before the first set_ema.
    void reset_ema();
    // Evaluation and export with the averaged weights, without a second network: flush_deferred(), ONE cnn_arena_swap of the arena
    // and the shadow, parameters_changed().  While swapped forward() (also under WithoutGrad), save_weights() -- the reference's
    // .model format, unchanged --, grad_cam() and params_device() see the average; a second call restores the training weights bit
    // for bit.  No misuse to guard against: every entry that steps or counts a micro-batch (both update_gradients forms,
    // train_step), set_ema, reset_ema, save_ema_state and load_ema_state swap back first.  A write to the arena from outside while
    // swapped lands in the AVERAGED copy.  Before the first set_ema(decay > 0) it does nothing.
    void swap_ema();
    bool ema_swapped() const { return ema.swapped; }
    data_type* ema_device() const { return ema.shadow; }  // null before the first set_ema(decay > 0)
    data_type ema_decay() const { return ema.decay; }
    uint64_t ema_updates() const { return ema.updates; }
    bool ema_active() const { return ema.decay > 0; }
    // The average beside a .model checkpoint and an optimizer state file (whose formats do not change): a header of magic "CNNAEMA1",
    // n_params, updates, decay, warmup, average_stats, then the shadow.  Status codes as save_ / load_optimizer_state: save 0 = ok,
    // 1 = cannot write, 4 = the average was never switched on (no shadow); load 0 = ok, 1 = cannot open, 2 = not such a file / truncated / options out of
    // range, 3 = written for another n_params; nothing is changed on failure, on success the file's options are set as by set_ema,
    // then its shadow and counter.  (A file may carry decay 0: an average that was switched off.)
    int save_ema_state(const std::filesystem::path& path);
    int load_ema_state(const std::filesystem::path& path);

protected:
    void invalidate_filter_images();  // (the part of parameters_changed() the container's own SGD step needs too)

public:
    // data parallelism over `world` replicas of this container (one per GPU), comm from cnn_comm_init_rank / _init_all:
    // backward() then leaves LOCAL gradients in the arena, update_gradients(lr) all-reduces them (RCCL, fp32 sum, on a
    // communication stream) and applies lr * (1/world) * sum.  Pass comm = nullptr to switch it off again.
    void set_comm(void* rccl_comm, int world);
    // sums the gradient arena over the replicas now (idempotent per backward pass); update_gradients(lr) calls it
    void allreduce_gradients();
    // One iteration of the reference's training loop (cnn.cpp:79-90: forward, softmax, cross_entroy_backward, backward,
    // update_gradients) that never leaves the device: the loss glue of func.cpp:16-73 runs as a kernel (fused into the last
    // LinearLayer's forward kernel when it has <= 8 outputs), nothing is copied back, the host never blocks.  labels_dev:
    // int32 [B] on the device.  The last layer must be a LinearLayer (the logits).  last_loss() fetches the loss of the most
    // recent step (-(1/B) * sum log p[label], func.cpp:67,71) -- the only call here that synchronises.
    void train_step(const std::vector<tensor>& input, const int* labels_dev, const data_type learning_rate);
    data_type last_loss();
    // Soft targets: label smoothing, mixup and CutMix without leaving the fused step.  The three entries below and train_step share one
    // body (run_step): the route -- fused loss head, fused step tail, deferred first-layer data gradient, every optimizer, clipping,
    // accumulation, the average, set_comm -- depends on none of them.  A step against soft targets runs the soft loss head
    // (cnn_linear_forward_softmax_xent_soft[_dx] where loss_head_supported(), cnn_linear_forward + cnn_softmax_xent_soft otherwise);
    // last_loss() works unchanged: -(1/B) * sum_b sum_j t[b][j] * log p[b][j], the terms added in sample order.
    //
    // set_label_smoothing(eps), eps in [0, 1) (anything else is reported and aborts, as in the other setters; 0, the default, is off):
    // every later train_step / forward_backward trains against the rows of cnn_soft_targets(labels, eps) -- (1 - eps) + eps / classes at
    // the label, eps / classes elsewhere.  They are built on the device into a container-owned [B][classes] buffer by ONE small launch at
    // the START of the step: it depends on nothing the step computes, so it never sits between the last convolution and the head.  With
    // eps == 0 the step is the hard-label one: the same kernels, the same launch log, the same bits.
    void set_label_smoothing(data_type eps);
    data_type label_smoothing() const { return smoothing; }
    // One step on a mixed batch: cnn_batch_mix of `input` into container-owned storage (mix.mode: CNN_MIX_MIXUP with mix.lam, or
    // CNN_MIX_CUTMIX with the box; mix.pair_rule / pair_shift choose the partners, inside this replica's batch under set_comm), the
    // targets lam * target(label) + (1 - lam) * target(partner's label) with the label smoothing set above, then the ordinary step.
    // MIXUP: lam = mix.lam.  CUTMIX: lam = cnn_cutmix_lambda(H, W, box) -- the container computes it, the caller's field cannot disagree
    // with the box.  A bad descriptor is reported by cnn_batch_mix and aborts like every failed library call.  Afterwards
    // Layer::get_output(), the input delta and grad_cam() describe the MIXED batch.  MEMORY: one extra input batch, allocated by the
    // first call and kept (154 MB at 256 x 3 x 224 x 224).
    void train_step_mixed(const std::vector<tensor>& input, const int* labels_dev, const cnn_mix_desc& mix, const data_type learning_rate);
    // One step against caller-provided dense targets, float [B][classes] on the device (distillation, per-sample mixing); the buffer
    // must stay untouched until the step's kernels have run (it is read by the head kernel).  Label smoothing does not apply.
    void train_step_soft(const std::vector<tensor>& input, const data_type* targets_dev, const data_type learning_rate);
    // the target rows of the last step that trained against soft targets ([B][classes], device); null before the first one
    const data_type* last_targets_device() const { return last_targets; }
    // Evaluation that never leaves the device (the reference's ClassificationEvaluator loop: forward, argmax, compare, on the host per
    // batch).  eval_begin / eval_step ... / eval_result; the arithmetic is cnn_eval_accumulate's (include/cnn_amd.h).
    // eval_begin(top_k): the class count is the last LinearLayer's out_features(); the first call allocates the state block
    // (cnn_eval_state_bytes), every call clears it (one cnn_memset_zero on architectures::stream) and sets k for the top-k count.
    // top_k outside [1, classes] is reported and aborts, as in the other setters.
    void eval_begin(int top_k = 1);
    // One batch: forward() with no_grad and lazy_host_sync set (both restored on every path), then ONE cnn_eval_accumulate on the
    // logits, on architectures::stream.  No D2H copy, no synchronise: it never blocks.  labels_dev: int32 [B] on the device; a label
    // outside [0, classes) -- the -1 of a padded last batch -- is counted as ignored and nowhere else.  Under no_grad BatchNorm2D uses
    // its moving statistics and Dropout scales.  It evaluates whatever the arena holds: after swap_ema() that is the average, and it
    // does not swap back.  On layer outputs it has exactly forward()'s effects and nothing else: parameters, gradients, the
    // accumulator and its phase, optimizer state, the step counter, the shadow and the moving statistics are untouched (like every
    // forward() it first orders a data gradient the last train_step deferred).  The [batch] prediction buffer is allocated by the
    // first step and grows with a larger batch.  Aborts with a message when eval_begin was never called.  Under set_comm every
    // replica counts ITS shard and nothing is exchanged: the caller adds the integers (and the loss sums) of the replicas.
    void eval_step(const std::vector<tensor>& input, const int* labels_dev);
    // the totals since eval_begin; like last_loss() it synchronises (cnn_eval_read).  confusion (optional) receives classes * classes
    // counts, row = label, column = prediction.
    EvalResult eval_result(std::vector<uint64_t>* confusion = nullptr);
    // int32 [B] predictions of the last eval_step (device); null before the first one
    const int* last_predictions_device() const { return eval_pred; }
    // TEST SUPPORT (tests/test_gpu_optimizer.py's host-stepped reference net; no product path calls it): train_step without its SGD
    // step, as the plain sequence (forward(), the loss kernel, backward(): no fused loss head, no fused step tail) -- the gradients of the
    // batch are left in the arena, last_loss() works.
    void forward_backward(const std::vector<tensor>& input, const int* labels_dev);
    const data_type* last_probs_device() const { return loss_probs.base; }
    // train_step defers the data gradient of a pool-fused first block (no consumer: alexnet.cpp:55 discards it) into the next
    // forward pass.  flush_deferred() launches a still-pending one and orders it before later work on architectures::stream; every
    // other entry point of the container does that itself, a caller only needs it before timing ends or before it reads that
    // layer's delta tensors through raw device pointers.
    void flush_deferred();
private:
    void ensure_loss_buffers(int B, int classes);
    // the body of every train step: labels_dev (hard labels) or targets_dev (dense targets), exactly one of them non-null
    void run_step(const std::vector<tensor>& input, const int* labels_dev, const data_type* targets_dev, const data_type learning_rate);
    // cnn_soft_targets into the container's buffer on architectures::stream; returns the buffer
    const data_type* build_targets(const int* labels_dev, int B, int classes, data_type lam, int pair_rule, int pair_shift);
    data_type smoothing = 0;
    data_type* target_rows = nullptr;          // [loss_batch][classes], allocated by the first step that needs it
    const data_type* last_targets = nullptr;
    // the mixed batch of train_step_mixed.  ONE buffer, rewritten by the next mixed step's first launch on architectures::stream: every
    // reader of a step's input is ordered on that stream before the step returns -- the first layer's forward and weight-gradient kernels
    // run on it (fused_tail launches the block's weight gradient there on both of its branches; the plain sequence, which clipping,
    // accumulation, the average and the bucketed exchange take, forks weight gradients to the library's side stream and joins it in
    // backward() / flush_bucket() before the step), the deferred data gradient reads d(pool), the mask and the filter image but not the
    // input, and a later get_output() re-computation is enqueued on the same stream before the next step's mix.
    BatchBuffer mixed_input;
    BatchBuffer mix_stage;  // (a host-resident input batch is staged here first)
    BatchBuffer loss_probs, loss_delta, logits_stage;   // [B][classes] each
    data_type* loss_terms = nullptr;      // [B] log p[label] (fused head) ...
    data_type* loss_sum = nullptr;        // ... or the ordered sum (unfused head); [1]
    bool loss_in_terms = false;
    int loss_batch = 0, loss_last_B = 0;
    // ---- evaluation on the device (eval_begin / eval_step / eval_result) ----
    void* eval_state = nullptr;   // cnn_eval_state_bytes(eval_classes) bytes, allocated by the first eval_begin
    int* eval_pred = nullptr;     // [eval_batch] predictions of the last eval_step
    int eval_classes = 0, eval_k = 1, eval_batch = 0;
};

// The reference's fixed network (alexnet.cpp:10-33).  forward / backward / update_gradients / save_weights / load_weights are
// declared on AlexNet itself like in the reference (architectures.h:203-213), so cpu/src/alexnet.cpp -- which DEFINES them --
// compiles against this header unchanged up to its OpenCV-typed grad_cam (:95, out of scope: SURVEY.md section 8f).
class AlexNet : public Sequential {
public:
    AlexNet(const int num_classes = 3, const bool batch_norm = false);
    // addition: adopt caller-provided device arenas (e.g. torch tensors) so the gradient arena can be all-reduced
    AlexNet(const int num_classes, data_type* params_dev, data_type* grads_dev, const bool batch_norm = false);
    std::vector<tensor> forward(const std::vector<tensor>& input);
    void backward(std::vector<tensor>& delta_start);
    void update_gradients(const data_type learning_rate = 1e-4);
    void update_gradients(const data_type learning_rate, const data_type grad_scale);
    void save_weights(const std::filesystem::path& save_path) const;
    void load_weights(const std::filesystem::path& checkpoint_path);
};

// BASELINE.json configs[3] / [4] as layer lists of the reference's own layer types (mirrored by cnn_amd/stacks.py):
// VGG-11-shaped: eight 3x3 stride-1 pad-1 convolutions 3->64->128->256->256->512->512->512->512, ReLU after each,
// MaxPool2D(2,2) after convolutions 1, 2, 4, 6, 8, LinearLayer(512*7*7 -> classes) for 224x224 inputs.
void build_vgg11(Sequential& net, const int num_classes = 3, const bool batch_norm = false);
// ResNet-18-shaped: the convolution shapes of ResNet-18 as a strictly sequential list (no residual adds: alexnet.cpp:41):
// 7x7 s2 p3 stem, MaxPool2D(2,2), four stages of four convolutions (3x3 s1 p1 inside a stage; stage entries 3x3 s2 p1,
// 1x1 s2, 3x3 s2 p1), BatchNorm2D + ReLU after every convolution, LinearLayer(512*7*7 -> classes).
void build_resnet18(Sequential& net, const int num_classes = 3, const bool batch_norm = true);
// MobileNet-V1-shaped (cnn_amd/stacks.py mobilenet_v1): 3x3 s2 p1 stem 3->32, the 13 blocks of DepthwiseConv2D(3x3, stride 1 or 2) +
// Conv2D(1x1), BatchNorm2D + ReLU after each of the two, MaxPool2D(7,7) in the average pool's place, LinearLayer(1024 -> classes).
void build_mobilenet_v1(Sequential& net, const int num_classes = 3, const bool batch_norm = true);

}  // namespace architectures

#endif  // CNN_AMD_ARCHITECTURES_H
