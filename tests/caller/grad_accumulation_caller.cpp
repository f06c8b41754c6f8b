// grad_accumulation_caller.cpp -- the loop a reference user writes to train on k micro-batches per optimizer step
// (Sequential::set_grad_accumulation), and the bare C ABI entry underneath (cnn_grad_accumulate) for a caller that keeps
// its own accumulator.  tests/test_grad_accumulation_compile.py compiles it against the public headers; nothing here is run.
#include <cstddef>
#include <vector>

#include "architectures.h"

// one epoch over `batches` micro-batches: the optimizer steps once per `micro_steps` of them, on the mean of their gradients
int accumulate_epoch(architectures::Sequential& net, const std::vector<std::vector<tensor> >& batches, const std::vector<const int*>& labels_dev,
                     const int micro_steps, const data_type learning_rate) {
    net.set_adam(0.9f, 0.999f, 1e-8f, 1e-2f, /*decoupled=*/true);
    net.set_grad_clip(1.f);
    net.set_grad_accumulation(micro_steps);
    int optimizer_steps = 0;
    for (size_t i = 0; i < batches.size(); ++i) {
        net.train_step(batches[i], labels_dev[i], learning_rate);  // calls 1 .. k-1 only add to the accumulator, call k steps
        if (net.accumulation_phase() == 0) ++optimizer_steps;
    }
    if (net.accumulation_phase() != 0) net.set_grad_accumulation(net.grad_accumulation());  // a ragged tail: the open window is discarded
    const data_type* window_sum = net.accumulated_grads_device();  // num_params() floats on the device
    net.set_grad_accumulation(1);                                  // off again: the fused step tail is back
    return window_sum != nullptr ? optimizer_steps : -1;
}

// the same with the caller's own accumulator and step: backward() leaves the micro-batch's gradients in the arena
int accumulate_by_hand(architectures::Sequential& net, float* acc_dev, const int micro_steps, const float learning_rate) {
    const size_t n = net.num_params();
    for (int phase = 0; phase < micro_steps; ++phase) {
        // ... forward(), the loss, backward() of micro-batch `phase` ...
        if (const int rc = cnn_grad_accumulate(acc_dev, net.grads_device(), n, /*first=*/phase == 0, architectures::stream)) return rc;
    }
    const int rc = cnn_sgd_update(net.params_device(), acc_dev, n, learning_rate, 1.f / (float)micro_steps, architectures::stream);
    net.parameters_changed();
    return rc;
}
