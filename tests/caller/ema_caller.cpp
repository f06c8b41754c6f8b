// ema_caller.cpp -- what a reference user writes to train with an exponential moving average of the weights and to evaluate / export
// the averaged model (Sequential::set_ema / swap_ema), and the bare C ABI entries underneath (cnn_ema_decay_at,
// cnn_ema_update, cnn_arena_swap) for a caller that keeps its own shadow.  tests/test_ema_compile.py compiles it against the public
// headers; nothing here is run.
#include <cstddef>
#include <cstdint>
#include <filesystem>
#include <vector>

#include "architectures.h"

// train with the average on, checkpoint the AVERAGED model in the reference's .model format, keep the average's state beside it
int train_and_export(architectures::Sequential& net, const std::vector<std::vector<tensor> >& batches, const std::vector<const int*>& labels_dev,
                     const std::vector<tensor>& validation, const data_type learning_rate, const std::filesystem::path& dir) {
    net.set_adam(0.9f, 0.999f, 1e-8f, 1e-2f, /*decoupled=*/true);
    net.set_ema(0.999f, /*warmup=*/true);
    for (size_t i = 0; i < batches.size(); ++i) net.train_step(batches[i], labels_dev[i], learning_rate);  // one update of the average per step
    if (!net.ema_active() || net.ema_updates() != batches.size() || net.ema_device() == nullptr) return -1;
    net.swap_ema();  // the arena now holds the average
    const bool swapped = net.ema_swapped();
    const std::vector<tensor> logits = net.forward(validation);
    net.save_weights(dir / "averaged.model");
    const data_type* averaged = net.params_device();
    net.swap_ema();  // back to the training weights, bit for bit (a train_step would have done it too)
    if (const int rc = net.save_ema_state(dir / "average.emastate")) return rc;
    net.load_weights(dir / "other.model");
    net.reset_ema();  // the average starts again from the loaded weights
    if (const int rc = net.load_ema_state(dir / "average.emastate")) return rc;
    net.set_ema(0);  // off: the shadow stays, nothing more is launched, the fused step tail is back
    return (swapped && !logits.empty() && averaged != nullptr && net.ema_decay() == 0) ? 0 : -1;
}

// the same with the caller's own shadow buffer: everything but the last `stats` floats is averaged
int average_by_hand(architectures::Sequential& net, float* shadow_dev, const uint64_t updates_done, const uint32_t stats) {
    const size_t n = net.num_params();
    const uint32_t ranges[2] = {0u, (uint32_t)n - stats};
    const float decay = cnn_ema_decay_at(0.9999f, /*warmup=*/1, updates_done);
    if (updates_done == 0) {  // decay 0: shadow = parameters, a copy of the bits
        if (const int rc = cnn_ema_update(shadow_dev, net.params_device(), n, 0.f, nullptr, nullptr, 0, architectures::stream)) return rc;
    }
    if (const int rc = cnn_ema_update(shadow_dev, net.params_device(), n, decay, ranges, nullptr, 1, architectures::stream)) return rc;
    const int rc = cnn_arena_swap(net.params_device(), shadow_dev, n, architectures::stream);  // evaluate with the average ...
    net.parameters_changed();
    return rc;  // ... and swap again afterwards
}
