// photo_caller.cpp -- the photometric half of a reference user's input pipeline on the device: beside the decoded bytes and the sampled
// map of augment_caller.cpp, a photo stager's slot takes 20 floats per image (architectures::PhotoAugmentor::make_photo: colour jitter
// and an erase box), and the stager carries the dataset's mean / std.  Underneath: cnn_colour_matrix of
// include/cnn_amd.h for a caller with a recipe of its own.  tests/test_photo_compile.py compiles it against the public headers; nothing
// here is run.
#include <cstddef>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "architectures.h"
#include "augment.h"

void* make_photo_stager(const int B, const int Hs, const int Ws, const int H, const int W) {
    void* stager = nullptr;
    if (cnn_batch_stager_create_u8_photo(&stager, B, Hs, Ws, H, W, /*depth=*/3)) return nullptr;
    const float mean[3] = {0.406f, 0.456f, 0.485f}, std[3] = {0.225f, 0.224f, 0.229f};  // ImageNet's, in cv::imread's BGR order
    if (cnn_batch_stager_set_normalize(stager, mean, std, /*clamp=*/1)) return nullptr;
    if (cnn_batch_stager_set_fill(stager, 0.f)) return nullptr;  // the border in output units: the mean colour
    return stager;
}

architectures::PhotoAugmentor make_photo_augmentor() {
    const std::vector<std::pair<std::string, float> > ops = {{"brightness", 0.8f}, {"contrast", 0.8f}, {"saturation", 0.8f}, {"hue", 0.5f},
                                                             {"erase", 0.25f}};
    architectures::PhotoAugmentor augmentor(ops, /*seed=*/7);
    augmentor.hue = 18.f;
    augmentor.erase_rand = true;
    return augmentor;
}

// one batch through the photo stager; returns the device fp32 [B][3][H][W] batch
const float* stage_photo_batch(void* stager, architectures::ImageAugmentor& geometric, architectures::PhotoAugmentor& photometric,
                               const std::vector<const unsigned char*>& images, const int Hs, const int Ws, const int H, const int W, int* slot_out) {
    void* host = nullptr;
    float* matrices = nullptr;
    float* photo = nullptr;
    void* dev = nullptr;
    if (cnn_batch_stager_acquire(stager, &host, slot_out)) return nullptr;
    if (cnn_batch_stager_matrices(stager, *slot_out, &matrices)) return nullptr;  // preset to the plain resize map
    if (cnn_batch_stager_photo(stager, *slot_out, &photo)) return nullptr;        // preset to the identity: no jitter, no box
    const size_t image_bytes = (size_t)Hs * Ws * 3;
    for (size_t b = 0; b < images.size(); ++b) {
        std::memcpy((unsigned char*)host + b * image_bytes, images[b], image_bytes);
        geometric.make_matrix(Hs, Ws, H, W, matrices + 6 * b);
        photometric.make_photo(H, W, photo + 20 * b);
    }
    if (cnn_batch_stager_submit(stager, *slot_out, &dev)) return nullptr;
    if (cnn_batch_stager_wait(stager, *slot_out, architectures::stream)) return nullptr;
    return (const float*)dev;  // cnn_batch_stager_release(stager, slot, stream) once the step that reads it is enqueued
}

// a fixed recipe by hand: the first twelve floats of every sample's block
int colour_by_hand(float* photo, const int B) {
    const cnn_colour_op ops[4] = {{CNN_COL_BRIGHTNESS, 1.2f, 0.f}, {CNN_COL_CONTRAST, 0.8f, 0.5f}, {CNN_COL_SATURATION, 1.1f, 0.f}, {CNN_COL_HUE, -10.f, 0.f}};
    for (int b = 0; b < B; ++b)
        if (const int rc = cnn_colour_matrix(ops, 4, photo + 20 * (size_t)b)) return rc;
    return 0;
}
