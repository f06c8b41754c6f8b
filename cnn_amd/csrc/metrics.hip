// metrics.hip -- evaluation on the device (an addition: the reference's ClassificationEvaluator runs on the host): loss, top-1 / top-k
// and confusion counts of a batch of logits accumulated into a device state block, and the one call that reads the block back.
// Layout of the block and the arithmetic: include/cnn_amd.h (cnn_eval_accumulate).
#include <cstdint>

#include "common.h"

using namespace cnn_amd;

namespace {

constexpr int kBlock = 256;
constexpr int kCounts = 4;  // samples, top-1 correct, top-k correct, ignored

// the block as the kernel sees it: counts[4], loss_sum, confusion[classes][classes] -- 8-byte words throughout
__device__ __forceinline__ unsigned long long* state_counts(void* state) { return (unsigned long long*)state; }
__device__ __forceinline__ double* state_loss(void* state) { return (double*)state + kCounts; }
__device__ __forceinline__ unsigned long long* state_confusion(void* state) { return (unsigned long long*)state + kCounts + 1; }

// softmax_xent_kernel's shape (elementwise.hip): one workgroup, thread t owns samples t, t+256, ...; a sample's max, sum and
// p[label] are that kernel's expressions in that order, and one lane adds the loss terms in ascending sample order, so the batch
// sum has its bits.  At 3 classes the kernel is a chain of memory round trips, so it is kept at the loss kernel's ONE: the label is
// requested beside the row and z[label] is picked up by the max loop (no load that waits for the label), lane 0 requests the old
// loss total before the rows (one workgroup per launch, launches of a stream in order: a plain load and store), and the integers go
// out as no-return vector atomics -- a wave's counts from its ballots, by its first lane; a confusion cell by the sample's lane.
__global__ __launch_bounds__(kBlock) void eval_accumulate_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                                 int32_t* __restrict__ pred, void* state, int B, int classes, int k) {
    __shared__ float terms[kBlock];
    double loss_before = 0.0;
    if (threadIdx.x == 0) loss_before = *state_loss(state);
    unsigned int wave_counts[kCounts] = {0, 0, 0, 0};  // (wave-uniform)
    float running = 0.f;
    for (int base = 0; base < B; base += kBlock) {
        const int b = base + threadIdx.x;
        float term = 0.f;  // (an ignored sample adds +0: the sum keeps its bits)
        bool counted = false, ignored = false, top1 = false, topk = false;
        if (b < B) {
            const int label = labels[b];
            const float* in = logits + (size_t)b * classes;
            float mx = in[0];  // Tensor3D::argmax = first maximum, strict '>'
            float zy = mx;     // z[label] once the loop has passed it (label 0: already)
            int best = 0;
            for (int i = 1; i < classes; ++i) {
                const float z = in[i];
                if (i == label) zy = z;
                if (z > mx) {
                    mx = z;
                    best = i;
                }
            }
            if (pred) pred[b] = best;
            ignored = label < 0 || label >= classes;
            if (!ignored) {
                float sum = 0.f;
                int rank = 0;
                for (int i = 0; i < classes; ++i) {
                    const float z = in[i];
                    sum += clamped_exp(z - mx);
                    rank += (z > zy || (i < label && z == zy)) ? 1 : 0;
                }
                float p = clamped_exp(zy - mx) / sum;
                if (isnan(p)) p = 0.f;
                term = logf(p);
                counted = true;
                top1 = best == label;
                topk = rank < k;
                atomicAdd(state_confusion(state) + (size_t)label * classes + best, 1ull);
            }
        }
        wave_counts[0] += __popcll(__ballot(counted));
        wave_counts[1] += __popcll(__ballot(top1));
        wave_counts[2] += __popcll(__ballot(topk));
        wave_counts[3] += __popcll(__ballot(ignored));
        terms[threadIdx.x] = term;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = min(kBlock, B - base);
            for (int i = 0; i < cnt; ++i) running += terms[i];
        }
        __syncthreads();
    }
    if (threadIdx.x % kWave == 0) {
#pragma unroll
        for (int c = 0; c < kCounts; ++c)
            if (wave_counts[c]) atomicAdd(state_counts(state) + c, (unsigned long long)wave_counts[c]);
    }
    if (threadIdx.x == 0) *state_loss(state) = loss_before + (double)(-running);
}

}  // namespace

extern "C" {

size_t cnn_eval_state_bytes(int classes) {
    if (classes <= 0) {
        fail(CNN_AMD_E_BADARG, "cnn_eval_state_bytes: classes=%d", classes);
        return 0;
    }
    return sizeof(uint64_t) * ((size_t)kCounts + 1 + (size_t)classes * classes);
}

int cnn_eval_accumulate(const float* logits, const int32_t* labels, int32_t* pred, void* state, int B, int classes, int k, void* stream) {
    CNN_REQUIRE(logits && labels && state, "cnn_eval_accumulate: null pointer");
    CNN_REQUIRE(B > 0 && classes > 0, "cnn_eval_accumulate: B=%d classes=%d", B, classes);
    CNN_REQUIRE(k >= 1 && k <= classes, "cnn_eval_accumulate: k=%d outside [1, classes=%d]", k, classes);
    hipStream_t s = as_stream(stream);
    CNN_KLAUNCH(s, "eval_accumulate", (eval_accumulate_kernel<<<1, kBlock, 0, s>>>(logits, labels, pred, state, B, classes, k)),
                "B=%d classes=%d k=%d", B, classes, k);
    return CNN_AMD_OK;
}

int cnn_eval_read(const void* state, int classes, cnn_eval_result* out, uint64_t* confusion, void* stream) {
    CNN_REQUIRE(state && out, "cnn_eval_read: null pointer");
    CNN_REQUIRE(classes > 0, "cnn_eval_read: classes=%d", classes);
    static_assert(sizeof(cnn_eval_result) == sizeof(uint64_t) * (kCounts + 1), "cnn_eval_result is the head of the state block");
    hipStream_t s = as_stream(stream);
    CNN_HIP_CHECK(hipMemcpyAsync(out, state, sizeof(cnn_eval_result), hipMemcpyDeviceToHost, s));
    if (confusion)
        CNN_HIP_CHECK(hipMemcpyAsync(confusion, (const uint64_t*)state + kCounts + 1, sizeof(uint64_t) * (size_t)classes * classes,
                                     hipMemcpyDeviceToHost, s));
    publish_mark_stale(s);
    CNN_HIP_CHECK(hipStreamSynchronize(s));
    return CNN_AMD_OK;
}

}  // extern "C"
