// augment_caller.cpp -- what a reference user writes in place of ImageAugmentor::make_augment on every cv::Mat of a batch
// (pipeline.cpp:40-77, 129-140): the decoded bytes go into a slot of an augmenting stager as they are, one sampled map per image goes
// beside them (architectures::ImageAugmentor::make_matrix), and flip / crop / rotate / resize happen on the device behind the upload
// (INTEGRATION.md).  Underneath: cnn_augment_matrix and cnn_augment_u8 of include/cnn_amd.h for a caller with device bytes of its own.
// tests/test_augment_compile.py compiles it against the public headers; nothing here is run.
#include <cstddef>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "architectures.h"
#include "augment.h"

// one batch through the stager: `images` are B decoded images of Hs x Ws x 3 bytes each; returns the device fp32 [B][3][H][W] batch
const float* stage_batch(void* stager, architectures::ImageAugmentor& augmentor, const std::vector<const unsigned char*>& images, const int Hs,
                         const int Ws, const int H, const int W, int* slot_out) {
    void* host = nullptr;
    float* matrices = nullptr;
    void* dev = nullptr;
    if (cnn_batch_stager_acquire(stager, &host, slot_out)) return nullptr;
    if (cnn_batch_stager_matrices(stager, *slot_out, &matrices)) return nullptr;  // preset to the plain resize map
    const size_t image_bytes = (size_t)Hs * Ws * 3;
    for (size_t b = 0; b < images.size(); ++b) {
        std::memcpy((unsigned char*)host + b * image_bytes, images[b], image_bytes);
        augmentor.make_matrix(Hs, Ws, H, W, matrices + 6 * b);
    }
    if (cnn_batch_stager_submit(stager, *slot_out, &dev)) return nullptr;
    if (cnn_batch_stager_wait(stager, *slot_out, architectures::stream)) return nullptr;
    return (const float*)dev;  // cnn_batch_stager_release(stager, slot, stream) once the step that reads it is enqueued
}

void* make_stager(const int B, const int Hs, const int Ws, const int H, const int W) {
    void* stager = nullptr;
    if (cnn_batch_stager_create_u8_aug(&stager, B, Hs, Ws, H, W, /*depth=*/3)) return nullptr;
    if (cnn_batch_stager_set_fill(stager, 0.5f)) return nullptr;  // the border of rotated corners: mid grey
    return stager;
}

architectures::ImageAugmentor make_augmentor() {
    const std::vector<std::pair<std::string, float> > ops = {{"hflip", 0.5f}, {"vflip", 0.2f}, {"crop", 0.7f}, {"rotate", 0.6f}};
    architectures::ImageAugmentor augmentor(ops);
    augmentor.max_angle = 10.f;
    return augmentor;
}

// the same on bytes that are on the device already: a fixed recipe for every image
int augment_by_hand(const unsigned char* src_dev, float* matrices_dev, float* dst_dev, const int B, const int Hs, const int Ws, const int H,
                    const int W) {
    const cnn_augment_op ops[3] = {{CNN_AUG_CROP, 8.f, 8.f, (float)(Ws - 16), (float)(Hs - 16)}, {CNN_AUG_HFLIP, 0.f, 0.f, 0.f, 0.f},
                                   {CNN_AUG_ROTATE, 90.f, 0.f, 0.f, 0.f}};
    std::vector<float> host((size_t)B * 6);
    for (int b = 0; b < B; ++b)
        if (const int rc = cnn_augment_matrix(ops, 3, Hs, Ws, H, W, host.data() + 6 * (size_t)b)) return rc;
    if (const int rc = cnn_memcpy_h2d(matrices_dev, host.data(), host.size() * sizeof(float), architectures::stream)) return rc;
    if (const int rc = cnn_stream_synchronize(architectures::stream)) return rc;  // (`host` is pageable and leaves scope)
    return cnn_augment_u8(src_dev, B, Hs, Ws, matrices_dev, /*fill=*/0.f, dst_dev, H, W, architectures::stream);
}
