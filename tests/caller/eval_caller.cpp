// eval_caller.cpp -- what a reference user writes in place of the ClassificationEvaluator loop (forward, argmax and compare on the host,
// per batch): Sequential::eval_begin / eval_step / eval_result, and the bare C ABI entries underneath
// (cnn_eval_state_bytes, cnn_eval_accumulate, cnn_eval_read) for a caller that has logits of its own.  tests/test_eval_compile.py
// compiles it against the public headers; nothing here is run.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "architectures.h"

// one pass over a validation set with the averaged weights; the last batch is padded with label -1 by the caller
double validate(architectures::Sequential& net, const std::vector<std::vector<tensor> >& batches, const std::vector<const int*>& labels_dev,
                std::vector<uint64_t>& confusion, double* top5_out) {
    net.swap_ema();  // (nothing before the first set_ema: the training weights are evaluated)
    net.eval_begin(/*top_k=*/5);
    for (size_t i = 0; i < batches.size(); ++i) net.eval_step(batches[i], labels_dev[i]);  // never blocks
    const int* predictions_of_last_batch = net.last_predictions_device();
    const architectures::EvalResult r = net.eval_result(&confusion);  // the one synchronise
    if (net.ema_swapped()) net.swap_ema();
    if (predictions_of_last_batch == nullptr || r.samples == 0) return -1;
    *top5_out = (double)r.topk / (double)r.samples;
    return r.ignored == 0 ? r.accuracy() : r.mean_loss();
}

// the same on logits the caller computed itself
int count_by_hand(const float* logits_dev, const int32_t* labels_dev, int32_t* pred_dev, const int B, const int classes, cnn_eval_result* out) {
    void* state = nullptr;
    const size_t bytes = cnn_eval_state_bytes(classes);
    if (bytes == 0) return 1;
    if (const int rc = cnn_device_alloc(&state, bytes)) return rc;
    if (const int rc = cnn_memset_zero(state, bytes, architectures::stream)) return rc;  // all-zero bytes: the empty state
    if (const int rc = cnn_eval_accumulate(logits_dev, labels_dev, pred_dev, state, B, classes, /*k=*/1, architectures::stream)) return rc;
    std::vector<uint64_t> confusion((size_t)classes * classes);
    if (const int rc = cnn_eval_read(state, classes, out, confusion.data(), architectures::stream)) return rc;
    return cnn_device_free(state);
}
