// soft_targets_caller.cpp -- what a reference user writes to train with label smoothing, mixup and CutMix, or against a teacher's
// probabilities, without leaving the fused step (Sequential::set_label_smoothing / train_step_mixed / train_step_soft),
// and the bare C ABI entries underneath for a caller with its own loop.  tests/test_soft_targets_compile.py compiles it against the
// public headers; nothing here is run.
#include <cstddef>
#include <vector>

#include "architectures.h"

// one epoch: label smoothing on every step, every other batch mixed -- mixup and CutMix in turn
data_type smoothed_and_mixed_epoch(architectures::Sequential& net, const std::vector<std::vector<tensor> >& batches,
                                   const std::vector<const int*>& labels_dev, const std::vector<float>& lams, const data_type learning_rate) {
    net.set_label_smoothing(0.1f);
    for (size_t i = 0; i < batches.size(); ++i) {
        const int H = batches[i][0]->H, W = batches[i][0]->W;
        cnn_mix_desc mix{};
        mix.pair_rule = CNN_PAIR_FLIP;
        if (i % 4 == 1) {
            mix.mode = CNN_MIX_MIXUP;
            mix.lam = lams[i];
            net.train_step_mixed(batches[i], labels_dev[i], mix, learning_rate);
        } else if (i % 4 == 3) {
            mix.mode = CNN_MIX_CUTMIX;  // (the container takes lam from the box: cnn_cutmix_lambda)
            mix.pair_rule = CNN_PAIR_ROLL;
            mix.pair_shift = 1;
            mix.y0 = H / 4, mix.y1 = 3 * H / 4, mix.x0 = W / 4, mix.x1 = 3 * W / 4;
            net.train_step_mixed(batches[i], labels_dev[i], mix, learning_rate);
        } else {
            net.train_step(batches[i], labels_dev[i], learning_rate);
        }
    }
    const data_type* rows = net.last_targets_device();  // [B][classes] of the last step
    const data_type loss = net.last_loss();
    net.set_label_smoothing(0);  // off: the hard-label step again
    return (rows != nullptr && net.label_smoothing() == 0) ? loss : -1;
}

// distillation: the teacher's probabilities are the targets
void distill(architectures::Sequential& student, const std::vector<tensor>& batch, const data_type* teacher_probs_dev, const data_type learning_rate) {
    student.train_step_soft(batch, teacher_probs_dev, learning_rate);
}

// the C ABI alone: a mixed batch, its targets, the generic soft loss
int by_hand(const float* batch_dev, float* mixed_dev, const int32_t* labels_dev, float* targets_dev, const float* logits_dev, float* delta_dev,
            float* loss_sum_dev, int B, int classes) {
    cnn_mix_desc mix{CNN_MIX_CUTMIX, 0.f, CNN_PAIR_FLIP, 0, 56, 168, 56, 168};
    if (const int rc = cnn_batch_mix(&mix, batch_dev, mixed_dev, B, 3, 224, 224, architectures::stream)) return rc;
    const float lam = cnn_cutmix_lambda(224, 224, mix.y0, mix.y1, mix.x0, mix.x1);
    if (const int rc = cnn_soft_targets(labels_dev, targets_dev, B, classes, 0.1f, lam, mix.pair_rule, mix.pair_shift, architectures::stream)) return rc;
    return cnn_softmax_xent_soft(logits_dev, targets_dev, nullptr, delta_dev, loss_sum_dev, B, classes, architectures::stream);
}
