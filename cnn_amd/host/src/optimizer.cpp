// optimizer.cpp -- the optimizer of architectures::Sequential (member functions; the class is in architectures.h): ONE kind
// (OptKind) says which step the container takes on its flat arena, every kind has its options struct, all kinds share one block of
// state (OptState), and the state files are one writer and one reader over a table of formats.  Clipping by the global gradient norm
// is orthogonal to the kind and sits at the end, with the setter of gradient accumulation over micro-batches and the exponential
// moving average of the parameters (its setters, the swap, its state file).
#include <algorithm>
#include <cassert>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "architectures.h"
#include "host_util.h"

using namespace architectures;
using cnn_amd_host::dev_alloc;
using cnn_amd_host::must;

// ---------------------------------------------------------------------------------------------------------------
// state: an arena of n_params floats is allocated and zeroed on first use, never zeroed by a switch
void Sequential::ensure_state_arena(data_type*& arena) {
    if (arena != nullptr) return;
    arena = (data_type*)dev_alloc(sizeof(data_type) * (n_params ? n_params : 1));
    must(cnn_memset_zero(arena, sizeof(data_type) * n_params, stream), "cnn_memset_zero");
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
}

// kSgdm / kAdam: where weight decay applies inside arena[lo, hi)
void Sequential::build_decay_table(DecayTable& t, size_t lo, size_t hi, const bool bias_and_norm) {
    t.lo = lo;
    t.hi = hi;
    t.host.clear();
    size_t idx = 0;
    Layer::RangeList local;
    for (const auto& layer : layers_sequence) {
        const size_t off = layer_offsets[idx++];
        local.clear();
        layer->decay_ranges(bias_and_norm, local);
        for (const auto& r : local) {
            const size_t b = std::max(off + r.first, lo), e = std::min(off + r.second, hi);
            if (b >= e) continue;
            if (!t.host.empty() && t.host.back() == (uint32_t)(b - lo)) t.host.back() = (uint32_t)(e - lo);  // (neighbours merge)
            else {
                t.host.push_back((uint32_t)(b - lo));
                t.host.push_back((uint32_t)(e - lo));
            }
        }
    }
    if (t.dev) {
        must(cnn_device_free(t.dev), "cnn_device_free");
        t.dev = nullptr;
    }
    if (t.host.size() / 2 > (size_t)CNN_SGD_INLINE_RANGES) {  // beyond what travels in the kernel arguments: the kernel reads a device copy
        t.dev = (uint32_t*)dev_alloc(sizeof(uint32_t) * t.host.size());
        must(cnn_memcpy_h2d(t.dev, t.host.data(), sizeof(uint32_t) * t.host.size(), stream), "cnn_memcpy_h2d");
        must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
    }
}

void Sequential::build_decay_tables(const bool bias_and_norm) {
    const size_t front = front_block_params();
    build_decay_table(opt.decay_tables[0], 0, n_params, bias_and_norm);
    build_decay_table(opt.decay_tables[1], front, n_params, bias_and_norm);
    build_decay_table(opt.decay_tables[2], 0, front, bias_and_norm);
}

// kLamb / kLars: the segment table -- every layer's param_tensors() at the layer's arena offset; DECAY where the decay policy
// (decay_ranges) covers the tensor, ADAPT on the first tensor of a Conv2D / LinearLayer (the weights) and, with adapt_bias_and_norm,
// wherever decay_ranges(true) reaches (biases, gamma / beta -- never the moving statistics)
void Sequential::build_segment_table(const bool decay_bias_and_norm, const bool adapt_bias_and_norm) {
    std::vector<uint32_t> bounds(1, 0u), flags;
    auto covered = [](const Layer::RangeList& ranges, size_t b, size_t e) {
        for (const auto& r : ranges)
            if (r.first <= b && e <= r.second) return true;
        return false;
    };
    size_t idx = 0;
    Layer::RangeList tensors, decayed, weights, all;
    for (const auto& layer : layers_sequence) {
        const size_t off = layer_offsets[idx++];
        tensors.clear();
        decayed.clear();
        weights.clear();
        all.clear();
        layer->param_tensors(tensors);
        layer->decay_ranges(decay_bias_and_norm, decayed);
        layer->decay_ranges(false, weights);
        layer->decay_ranges(true, all);
        size_t at = 0;
        for (const auto& t : tensors) {
            assert(t.first == at && t.second > t.first && "param_tensors() tiles the layer's parameter block");
            at = t.second;
            uint32_t f = 0;
            if (covered(decayed, t.first, t.second)) f |= CNN_SEG_DECAY;
            if (covered(adapt_bias_and_norm ? all : weights, t.first, t.second)) f |= CNN_SEG_ADAPT;
            bounds.push_back((uint32_t)(off + t.second));
            flags.push_back(f);
        }
        assert(at == layer->param_count() && "param_tensors() tiles the layer's parameter block");
        (void)at;  // (read by the asserts only)
    }
    assert(flags.empty() ? n_params == 0 : bounds.back() == n_params);
    if (opt.layerwise != nullptr && bounds == opt.seg_bounds && flags == opt.seg_flags) return;
    if (opt.layerwise != nullptr) {
        must(cnn_layerwise_destroy(opt.layerwise), "cnn_layerwise_destroy");
        opt.layerwise = nullptr;
    }
    opt.seg_bounds = bounds;
    opt.seg_flags = flags;
    if (!flags.empty())
        must(cnn_layerwise_create(opt.seg_bounds.data(), opt.seg_flags.data(), opt.seg_flags.size(), &opt.layerwise), "cnn_layerwise_create");
}

bool Sequential::trust_stats(std::vector<data_type>& w_norm, std::vector<data_type>& u_norm, std::vector<data_type>& ratio) {
    if (opt.layerwise == nullptr) return false;
    const size_t ns = opt.seg_flags.size();
    float* dev = nullptr;
    must(cnn_layerwise_stats(opt.layerwise, &dev), "cnn_layerwise_stats");
    std::vector<data_type> host(3 * ns);
    must(cnn_memcpy_d2h(host.data(), dev, sizeof(data_type) * host.size(), stream), "cnn_memcpy_d2h");
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
    w_norm.assign(host.begin(), host.begin() + ns);
    u_norm.assign(host.begin() + ns, host.begin() + 2 * ns);
    ratio.assign(host.begin() + 2 * ns, host.end());
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// the setters: begin the switch, make sure the kind's state exists, keep the options, build the kind's table, assign the kind.
// The two conditions every setter depends on -- a finalized container, an arena the 32-bit tables can index -- were one assert each
// per setter; here they are checked in every build, NDEBUG included, because a setter that went on would write through null arenas.
namespace {
// the option range of set_adam and set_lamb (their asserts, and the check of a state file's header: a NaN fails it)
bool moment_options_ok(data_type beta1, data_type beta2, data_type eps, data_type weight_decay) {
    return beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps > 0 && weight_decay >= 0;
}
}  // namespace

void Sequential::begin_optimizer_switch(const char* setter, const bool builds_32bit_table) {
    if (!finalized) {
        std::fprintf(stderr, "cnn_amd host: %s works on the flat arena: call finalize() first\n", setter);
        std::abort();
    }
    if (builds_32bit_table && n_params >= ((size_t)1 << 32) - 1024) {
        std::fprintf(stderr, "cnn_amd host: %s: the decay-range / segment tables are 32-bit, the arena has %zu parameters\n", setter, n_params);
        std::abort();
    }
    flush_deferred();  // (a side-stream tail of the previous step may still step the arena or read the tables rebuilt by the setter)
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
}

void Sequential::set_optimizer(const data_type momentum, const data_type weight_decay, const bool nesterov, const bool decay_bias_and_norm) {
    assert(momentum >= 0 && weight_decay >= 0);
    begin_optimizer_switch("set_optimizer");
    ensure_state_arena(opt.velocity);
    sgdm_opt = {{0, momentum, weight_decay, nesterov ? 1 : 0}, decay_bias_and_norm};
    build_decay_tables(decay_bias_and_norm);
    opt_kind = (momentum != 0 || weight_decay != 0) ? OptKind::kSgdm : OptKind::kPlain;
}

void Sequential::set_adam(const data_type beta1, const data_type beta2, const data_type eps, const data_type weight_decay, const bool decoupled,
                          const bool decay_bias_and_norm) {
    assert(moment_options_ok(beta1, beta2, eps, weight_decay));
    begin_optimizer_switch("set_adam");
    ensure_state_arena(opt.exp_avg);  // (opt.step starts at 0 and is never reset)
    ensure_state_arena(opt.exp_avg_sq);
    adam_opt = {{0, beta1, beta2, eps, weight_decay, decoupled ? 1 : 0, 0}, decay_bias_and_norm};
    build_decay_tables(decay_bias_and_norm);
    opt_kind = OptKind::kAdam;
}

void Sequential::set_lamb(const data_type beta1, const data_type beta2, const data_type eps, const data_type weight_decay, const bool decay_bias_and_norm,
                          const bool adapt_bias_and_norm) {
    assert(moment_options_ok(beta1, beta2, eps, weight_decay));
    begin_optimizer_switch("set_lamb");
    ensure_state_arena(opt.exp_avg);  // (opt.step starts at 0 and is never reset)
    ensure_state_arena(opt.exp_avg_sq);
    if (opt.lamb_update == nullptr) opt.lamb_update = (data_type*)dev_alloc(sizeof(data_type) * (n_params ? n_params : 1));
    lamb_opt = {{0, beta1, beta2, eps, weight_decay, 0}, decay_bias_and_norm, adapt_bias_and_norm};
    build_segment_table(decay_bias_and_norm, adapt_bias_and_norm);
    opt_kind = OptKind::kLamb;
}

void Sequential::set_lars(const data_type momentum, const data_type weight_decay, const data_type trust_coefficient, const data_type eps,
                          const bool nesterov, const bool decay_bias_and_norm, const bool adapt_bias_and_norm) {
    assert(momentum >= 0 && weight_decay >= 0 && trust_coefficient > 0 && eps > 0);
    begin_optimizer_switch("set_lars");
    ensure_state_arena(opt.velocity);
    lars_opt = {{0, momentum, weight_decay, trust_coefficient, eps, nesterov ? 1 : 0}, decay_bias_and_norm, adapt_bias_and_norm};
    build_segment_table(decay_bias_and_norm, adapt_bias_and_norm);
    opt_kind = OptKind::kLars;
}

// ---------------------------------------------------------------------------------------------------------------
// the step of the active kind on arena[lo, hi).  The caller has advanced opt.step once for this container step (update_gradients,
// fused_tail): the two range launches of the fused tail carry the same number.
// kSgdm / kAdam step the three ranges the setters built decay tables for, kLamb / kLars the whole arena, and no other
namespace {
[[noreturn]] void cannot_step(size_t lo, size_t hi) {
    std::fprintf(stderr, "cnn_amd host: step_arena: the active optimizer does not step arena[%zu, %zu)\n", lo, hi);
    std::abort();
}
}  // namespace

const Sequential::DecayTable& Sequential::decay_table_of(const size_t lo, const size_t hi) const {
    for (const auto& t : opt.decay_tables)
        if (t.lo == lo && t.hi == hi) return t;
    cannot_step(lo, hi);
}

void Sequential::step_arena(const size_t lo, const size_t hi, const data_type learning_rate, const data_type grad_scale, void* on_stream) {
    if (hi <= lo) return;
    const size_t n = hi - lo;
    data_type *p = param_arena + lo, *g = step_grads() + lo, *prev = param_prev + lo;
    switch (opt_kind) {
        case OptKind::kPlain:  // the reference's w -= lr * g
            must(cnn_sgd_update_keep(p, g, n, learning_rate, grad_scale, prev, on_stream), "cnn_sgd_update_keep");
            return;
        case OptKind::kSgdm: {
            const DecayTable& t = decay_table_of(lo, hi);
            sgdm_opt.abi.lr = learning_rate;
            must(cnn_sgd_momentum_update(p, g, opt.velocity + lo, n, &sgdm_opt.abi, grad_scale, t.host.data(), t.dev, t.host.size() / 2, prev,
                                         on_stream),
                 "cnn_sgd_momentum_update");
            return;
        }
        case OptKind::kAdam: {
            const DecayTable& t = decay_table_of(lo, hi);
            adam_opt.abi.lr = learning_rate;
            adam_opt.abi.step = opt.step;
            must(cnn_adam_update(p, g, opt.exp_avg + lo, opt.exp_avg_sq + lo, n, &adam_opt.abi, grad_scale, t.host.data(), t.dev,
                                 t.host.size() / 2, prev, on_stream),
                 "cnn_adam_update");
            return;
        }
        case OptKind::kLamb:
            if (lo != 0 || hi != n_params) cannot_step(lo, hi);
            lamb_opt.abi.lr = learning_rate;
            lamb_opt.abi.step = opt.step;
            must(cnn_lamb_update(opt.layerwise, p, g, opt.exp_avg, opt.exp_avg_sq, opt.lamb_update, &lamb_opt.abi, grad_scale, prev, on_stream),
                 "cnn_lamb_update");
            return;
        case OptKind::kLars:
            if (lo != 0 || hi != n_params) cannot_step(lo, hi);
            lars_opt.abi.lr = learning_rate;
            must(cnn_lars_update(opt.layerwise, p, g, opt.velocity, &lars_opt.abi, grad_scale, prev, on_stream), "cnn_lars_update");
            return;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// state files.  Four formats, byte for byte what the commits that introduced each optimizer wrote: a header -- magic, n_params,
// [step,] the setter's options as float / uint32 in the setter's argument order -- then the kind's state arenas, n_params floats each.
namespace {
struct OptStateHeader {  // momentum SGD, and the plain step as momentum 0, weight decay 0; then the velocity
    char magic[8];
    uint64_t n_params;
    float momentum, weight_decay;
    uint32_t nesterov, decay_bias_and_norm;
};
struct AdamStateHeader {  // then exp_avg, exp_avg_sq
    char magic[8];
    uint64_t n_params, step;
    float beta1, beta2, eps, weight_decay;
    uint32_t decoupled, decay_bias_and_norm;
};
struct LambStateHeader {  // then exp_avg, exp_avg_sq
    char magic[8];
    uint64_t n_params, step;
    float beta1, beta2, eps, weight_decay;
    uint32_t decay_bias_and_norm, adapt_bias_and_norm;
};
struct LarsStateHeader {  // then the velocity
    char magic[8];
    uint64_t n_params;
    float momentum, weight_decay, trust_coefficient, eps;
    uint32_t nesterov, decay_bias_and_norm, adapt_bias_and_norm, pad;  // (pad: written as 0)
};
union StateHeader {  // (magic and n_params sit at the same place in all four)
    OptStateHeader sgdm;
    AdamStateHeader adam;
    LambStateHeader lamb;
    LarsStateHeader lars;
};
// the layouts are the file formats: pinned field by field
#define PIN(H, f, at) static_assert(offsetof(H, f) == at, #H "::" #f " moved: the state file's layout is fixed")
#define PIN3(H, f0, a0, f1, a1, f2, a2) PIN(H, f0, a0); PIN(H, f1, a1); PIN(H, f2, a2)
static_assert(sizeof(OptStateHeader) == 32, "the momentum state file's header is 32 bytes");
PIN3(OptStateHeader, magic, 0, n_params, 8, momentum, 16);
PIN3(OptStateHeader, weight_decay, 20, nesterov, 24, decay_bias_and_norm, 28);
static_assert(sizeof(AdamStateHeader) == 48, "the Adam state file's header is 48 bytes");
PIN3(AdamStateHeader, magic, 0, n_params, 8, step, 16);
PIN3(AdamStateHeader, beta1, 24, beta2, 28, eps, 32);
PIN3(AdamStateHeader, weight_decay, 36, decoupled, 40, decay_bias_and_norm, 44);
static_assert(sizeof(LambStateHeader) == 48, "the LAMB state file's header is 48 bytes");
PIN3(LambStateHeader, magic, 0, n_params, 8, step, 16);
PIN3(LambStateHeader, beta1, 24, beta2, 28, eps, 32);
PIN3(LambStateHeader, weight_decay, 36, decay_bias_and_norm, 40, adapt_bias_and_norm, 44);
static_assert(sizeof(LarsStateHeader) == 48, "the LARS state file's header is 48 bytes");
PIN3(LarsStateHeader, magic, 0, n_params, 8, momentum, 16);
PIN3(LarsStateHeader, weight_decay, 20, trust_coefficient, 24, eps, 28);
PIN3(LarsStateHeader, nesterov, 32, decay_bias_and_norm, 36, adapt_bias_and_norm, 40);
PIN(LarsStateHeader, pad, 44);
#undef PIN3
#undef PIN
}  // namespace

// One format: what identifies it, which arenas follow the header, how the options go into the header (`fill`; magic and n_params are the
// writer's), whether a header read from a file holds options the setter accepts (`valid`: comparisons that a NaN fails), and how it
// becomes the active optimizer (`activate`: the setter, then the step counter).
struct Sequential::StateFormat {
    OptKind kind;  // (kPlain is saved in kSgdm's format)
    const char* magic;
    size_t header_bytes;
    size_t n_arenas;
    data_type* OptState::*arenas[2];
    void (*fill)(const Sequential& net, StateHeader& h);
    bool (*valid)(const StateHeader& h);
    void (*activate)(Sequential& net, const StateHeader& h);
    static const StateFormat all[4];
};

const Sequential::StateFormat Sequential::StateFormat::all[4] = {
    {OptKind::kSgdm, "CNNAOPT1", sizeof(OptStateHeader), 1, {&OptState::velocity, nullptr},
     [](const Sequential& net, StateHeader& h) {
         const auto& o = net.sgdm_opt;
         h.sgdm = {{}, 0, o.abi.momentum, o.abi.weight_decay, o.abi.nesterov != 0, o.decay_bias_and_norm};
     },
     [](const StateHeader& h) { return h.sgdm.momentum >= 0 && h.sgdm.weight_decay >= 0; },
     [](Sequential& net, const StateHeader& h) {
         net.set_optimizer(h.sgdm.momentum, h.sgdm.weight_decay, h.sgdm.nesterov != 0, h.sgdm.decay_bias_and_norm != 0);
     }},
    {OptKind::kAdam, "CNNAADM1", sizeof(AdamStateHeader), 2, {&OptState::exp_avg, &OptState::exp_avg_sq},
     [](const Sequential& net, StateHeader& h) {
         const auto& o = net.adam_opt;
         h.adam = {{}, 0, net.opt.step, o.abi.beta1, o.abi.beta2, o.abi.eps, o.abi.weight_decay, o.abi.decoupled != 0, o.decay_bias_and_norm};
     },
     [](const StateHeader& h) { return moment_options_ok(h.adam.beta1, h.adam.beta2, h.adam.eps, h.adam.weight_decay); },
     [](Sequential& net, const StateHeader& h) {
         net.set_adam(h.adam.beta1, h.adam.beta2, h.adam.eps, h.adam.weight_decay, h.adam.decoupled != 0, h.adam.decay_bias_and_norm != 0);
         net.opt.step = h.adam.step;
     }},
    {OptKind::kLamb, "CNNALMB1", sizeof(LambStateHeader), 2, {&OptState::exp_avg, &OptState::exp_avg_sq},
     [](const Sequential& net, StateHeader& h) {
         const auto& o = net.lamb_opt;
         h.lamb = {{}, 0, net.opt.step, o.abi.beta1, o.abi.beta2, o.abi.eps, o.abi.weight_decay, o.decay_bias_and_norm, o.adapt_bias_and_norm};
     },
     [](const StateHeader& h) { return moment_options_ok(h.lamb.beta1, h.lamb.beta2, h.lamb.eps, h.lamb.weight_decay); },
     [](Sequential& net, const StateHeader& h) {
         net.set_lamb(h.lamb.beta1, h.lamb.beta2, h.lamb.eps, h.lamb.weight_decay, h.lamb.decay_bias_and_norm != 0, h.lamb.adapt_bias_and_norm != 0);
         net.opt.step = h.lamb.step;
     }},
    {OptKind::kLars, "CNNALRS1", sizeof(LarsStateHeader), 1, {&OptState::velocity, nullptr},
     [](const Sequential& net, StateHeader& h) {
         const auto& o = net.lars_opt;
         h.lars = {{}, 0, o.abi.momentum, o.abi.weight_decay, o.abi.trust_coefficient, o.abi.eps, o.abi.nesterov != 0, o.decay_bias_and_norm,
                   o.adapt_bias_and_norm, 0};
     },
     [](const StateHeader& h) { return h.lars.momentum >= 0 && h.lars.weight_decay >= 0 && h.lars.trust_coefficient > 0 && h.lars.eps > 0; },
     [](Sequential& net, const StateHeader& h) {
         net.set_lars(h.lars.momentum, h.lars.weight_decay, h.lars.trust_coefficient, h.lars.eps, h.lars.nesterov != 0,
                      h.lars.decay_bias_and_norm != 0, h.lars.adapt_bias_and_norm != 0);
     }},
};

int Sequential::save_optimizer_state(const std::filesystem::path& path) {
    assert(finalized);
    const OptKind saved_as = opt_kind == OptKind::kPlain ? OptKind::kSgdm : opt_kind;
    const StateFormat* f = nullptr;
    for (const auto& cand : StateFormat::all)
        if (cand.kind == saved_as) f = &cand;
    if (opt.*(f->arenas[0]) == nullptr) return 4;  // (only kPlain can lack its format's arena: no setter was ever called)
    flush_deferred();
    std::vector<data_type> host(f->n_arenas * n_params);
    for (size_t a = 0; a < f->n_arenas; ++a)
        must(cnn_memcpy_d2h(host.data() + a * n_params, opt.*(f->arenas[a]), sizeof(data_type) * n_params, stream), "cnn_memcpy_d2h");
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
    StateHeader h;
    std::memset(&h, 0, sizeof(h));
    f->fill(*this, h);
    std::memcpy(h.sgdm.magic, f->magic, 8);
    h.sgdm.n_params = n_params;
    std::ofstream writer(path.c_str(), std::ios::binary);
    writer.write((const char*)&h, f->header_bytes);
    writer.write((const char*)host.data(), sizeof(data_type) * host.size());
    writer.close();
    return writer.good() ? 0 : 1;
}

// Nothing is changed on any failure: the header is checked and the whole payload read before the setter runs -- before any arena is
// allocated and before the step counter is touched.
int Sequential::load_optimizer_state(const std::filesystem::path& path) {
    assert(finalized);
    std::ifstream reader(path.c_str(), std::ios::binary);
    if (!reader.good()) return 1;
    StateHeader h;
    std::memset(&h, 0, sizeof(h));
    reader.read((char*)&h, 8);
    const StateFormat* f = nullptr;
    for (const auto& cand : StateFormat::all)
        if (reader.good() && std::memcmp(h.sgdm.magic, cand.magic, 8) == 0) f = &cand;
    if (f == nullptr) return 2;
    reader.read((char*)&h + 8, f->header_bytes - 8);
    if (!reader.good()) return 2;
    if (h.sgdm.n_params != (uint64_t)n_params) return 3;
    if (!f->valid(h)) return 2;
    std::vector<data_type> host(f->n_arenas * n_params);
    reader.read((char*)host.data(), sizeof(data_type) * host.size());
    if ((size_t)reader.gcount() != sizeof(data_type) * host.size()) return 2;
    f->activate(*this, h);
    for (size_t a = 0; a < f->n_arenas; ++a)
        must(cnn_memcpy_h2d(opt.*(f->arenas[a]), host.data() + a * n_params, sizeof(data_type) * n_params, stream), "cnn_memcpy_h2d");
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// clipping by the global gradient norm: in front of whichever step is active (update_gradients)
void Sequential::set_grad_clip(const data_type max_norm) {
    assert(finalized && "set_grad_clip works on the flat arena: call finalize() first");
    assert(max_norm >= 0);
    flush_deferred();  // (a side-stream tail of the previous step is ordered before the first clipped step's plain sequence)
    if (max_norm > 0 && clip_stats == nullptr) {
        clip_workspace_bytes = cnn_clip_grad_norm_workspace_bytes(n_params);
        clip_workspace = dev_alloc(clip_workspace_bytes);
        clip_stats = (data_type*)dev_alloc(sizeof(data_type) * 2);
        must(cnn_memset_zero(clip_stats, sizeof(data_type) * 2, stream), "cnn_memset_zero");
    }
    clip_max_norm = max_norm;
}

// ---------------------------------------------------------------------------------------------------------------
// gradient accumulation over micro-batches: which gradients the exchange, the clip and the step read (step_grads()), and how many
// container steps make one of them (count_micro_batch(), sequential.cpp)
void Sequential::set_grad_accumulation(const int micro_steps) {
    if (micro_steps < 1) {
        std::fprintf(stderr, "cnn_amd host: set_grad_accumulation: micro_steps=%d, at least 1 (1 = off)\n", micro_steps);
        std::abort();
    }
    begin_optimizer_switch("set_grad_accumulation", /*builds_32bit_table=*/false);
    if (micro_steps > 1) ensure_state_arena(accum_grads);  // (zeroed once; a window's first micro-batch overwrites it)
    accum_k = micro_steps;
    accum_phase = 0;  // (an open window is discarded)
}

data_type Sequential::last_grad_norm(data_type* coef_out) {
    assert(clip_stats != nullptr && "last_grad_norm: clipping was never switched on (set_grad_clip)");
    data_type host[2] = {0, 0};
    must(cnn_memcpy_d2h(host, clip_stats, sizeof(host), stream), "cnn_memcpy_d2h");
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
    if (coef_out) *coef_out = host[1];
    return host[0];
}

// ---------------------------------------------------------------------------------------------------------------
// exponential moving average of the parameters: a shadow arena behind every optimizer step (clip_and_step(), sequential.cpp), swapped
// into the parameter arena for evaluation and export
void Sequential::build_ema_table(const bool average_stats) {
    if (!average_stats) {  // weights, biases, gamma / beta -- everything but BatchNorm2D's moving statistics
        build_decay_table(ema.table, 0, n_params, /*bias_and_norm=*/true);
        return;
    }
    build_decay_table(ema.table, 0, 0, true);  // (empties the table and frees a device copy)
    ema.table.hi = n_params;
    if (n_params > 0) ema.table.host = {0u, (uint32_t)n_params};
}

void Sequential::fill_ema_shadow() {
    if (n_params > 0) must(cnn_ema_update(ema.shadow, param_arena, n_params, 0.f, nullptr, nullptr, 0, stream), "cnn_ema_update");
    ema.updates = 0;
}

void Sequential::set_ema(const data_type decay, const bool warmup, const bool average_stats) {
    if (!(decay >= 0 && decay < 1)) {
        std::fprintf(stderr, "cnn_amd host: set_ema: decay=%g outside [0, 1) (0 = off)\n", (double)decay);
        std::abort();
    }
    begin_optimizer_switch("set_ema");
    unswap_ema();
    build_ema_table(average_stats);
    ema.warmup = warmup;
    ema.average_stats = average_stats;
    if (decay > 0 && ema.shadow == nullptr) {
        ema.shadow = (data_type*)dev_alloc(sizeof(data_type) * (n_params ? n_params : 1));
        fill_ema_shadow();
    }
    ema.decay = decay;
}

void Sequential::reset_ema() {
    if (ema.shadow == nullptr) return;
    flush_deferred();
    unswap_ema();
    fill_ema_shadow();
}

void Sequential::swap_ema() {
    if (ema.shadow == nullptr) return;
    flush_deferred();
    if (n_params > 0) must(cnn_arena_swap(param_arena, ema.shadow, n_params, stream), "cnn_arena_swap");
    ema.swapped = !ema.swapped;
    parameters_changed();
}

namespace {
struct EmaStateHeader {  // then the shadow, n_params floats
    char magic[8];
    uint64_t n_params, updates;
    float decay;
    uint32_t warmup, average_stats, pad;  // (pad: written as 0)
};
static_assert(sizeof(EmaStateHeader) == 40 && offsetof(EmaStateHeader, updates) == 16 && offsetof(EmaStateHeader, decay) == 24 &&
                  offsetof(EmaStateHeader, warmup) == 28 && offsetof(EmaStateHeader, average_stats) == 32 && offsetof(EmaStateHeader, pad) == 36,
              "the EMA state file's header is 40 bytes, its layout is fixed");
const char kEmaMagic[9] = "CNNAEMA1";
}  // namespace

int Sequential::save_ema_state(const std::filesystem::path& path) {
    assert(finalized);
    if (ema.shadow == nullptr) return 4;
    flush_deferred();
    unswap_ema();
    std::vector<data_type> host(n_params);
    must(cnn_memcpy_d2h(host.data(), ema.shadow, sizeof(data_type) * n_params, stream), "cnn_memcpy_d2h");
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
    EmaStateHeader h;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.magic, kEmaMagic, 8);
    h.n_params = n_params;
    h.updates = ema.updates;
    h.decay = ema.decay;
    h.warmup = ema.warmup;
    h.average_stats = ema.average_stats;
    std::ofstream writer(path.c_str(), std::ios::binary);
    writer.write((const char*)&h, sizeof(h));
    writer.write((const char*)host.data(), sizeof(data_type) * host.size());
    writer.close();
    return writer.good() ? 0 : 1;
}

// Nothing is changed on any failure: the header is checked and the whole payload read before the setter runs.
int Sequential::load_ema_state(const std::filesystem::path& path) {
    assert(finalized);
    std::ifstream reader(path.c_str(), std::ios::binary);
    if (!reader.good()) return 1;
    EmaStateHeader h;
    std::memset(&h, 0, sizeof(h));
    reader.read((char*)&h, sizeof(h));
    if (!reader.good() || std::memcmp(h.magic, kEmaMagic, 8) != 0) return 2;
    if (h.n_params != (uint64_t)n_params) return 3;
    if (!(h.decay >= 0 && h.decay < 1) || h.warmup > 1 || h.average_stats > 1 || h.pad != 0) return 2;
    std::vector<data_type> host(n_params);
    reader.read((char*)host.data(), sizeof(data_type) * host.size());
    if ((size_t)reader.gcount() != sizeof(data_type) * host.size()) return 2;
    set_ema(h.decay, h.warmup != 0, h.average_stats != 0);  // (swaps back first)
    if (ema.shadow == nullptr) ema.shadow = (data_type*)dev_alloc(sizeof(data_type) * (n_params ? n_params : 1));  // (a file with decay 0)
    must(cnn_memcpy_h2d(ema.shadow, host.data(), sizeof(data_type) * n_params, stream), "cnn_memcpy_h2d");
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
    ema.updates = h.updates;
    return 0;
}
