// augment.h -- the reference's ImageAugmentor (cpu/include/pipeline.h, pipeline.cpp:40-77) for the device path: constructed like the
// reference's, from op names and probabilities, but instead of transforming a cv::Mat on the host it SAMPLES the same decisions and
// composes them into the six floats of one output -> source map (cnn_augment_matrix, include/cnn_amd.h).  A caller fills a slot of an
// augmenting stager (cnn_batch_stager_create_u8_aug) with one such map per image; the gather itself runs on the device, fused with the
// bytes -> fp32 conversion.  Header only; errors from the C ABI abort, like the reference's asserts.
#ifndef CNN_AMD_AUGMENT_H
#define CNN_AMD_AUGMENT_H

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <utility>
#include <vector>

extern "C" {
#include "cnn_amd.h"
}

namespace architectures {

class ImageAugmentor {
public:
    // op names: "hflip", "vflip", "crop", "rotate" (the reference's); second = the probability that the op fires for an image
    explicit ImageAugmentor(const std::vector<std::pair<std::string, float> >& _ops = {{"hflip", 0.5f}, {"vflip", 0.2f}, {"crop", 0.7f}, {"rotate", 0.5f}},
                            const unsigned seed = 212)
        : ops(_ops), engine(seed), crop_engine(seed + 1), rotate_engine(seed + 2), minus_engine(seed + 3) {}

    // One image's map: the ops in a shuffled order, each firing with its own probability; crop: a ratio uniform in [crop_min, 1] of the
    // current canvas at a uniform position; rotate: an angle uniform in [-max_angle, max_angle] degrees.  Then the resize to W x H.
    void make_matrix(const int Hs, const int Ws, const int H, const int W, float m[6]) {
        std::shuffle(ops.begin(), ops.end(), engine);
        std::vector<cnn_augment_op> chosen;
        int cw = Ws, ch = Hs;
        for (const auto& item : ops) {
            if (!(engine_float(engine) < item.second)) continue;
            cnn_augment_op op = {0, 0.f, 0.f, 0.f, 0.f};
            if (item.first == "hflip") op.kind = CNN_AUG_HFLIP;
            else if (item.first == "vflip") op.kind = CNN_AUG_VFLIP;
            else if (item.first == "crop") {
                const float ratio = crop_min + (1.f - crop_min) * engine_float(crop_engine);
                const int w = std::max(1, (int)(cw * ratio)), h = std::max(1, (int)(ch * ratio));
                op.kind = CNN_AUG_CROP;
                op.a = (float)std::uniform_int_distribution<int>(0, cw - w)(crop_engine);
                op.b = (float)std::uniform_int_distribution<int>(0, ch - h)(crop_engine);
                op.c = (float)w;
                op.d = (float)h;
                cw = w; ch = h;
            } else if (item.first == "rotate") {
                const float angle = max_angle * engine_float(rotate_engine);
                op.kind = CNN_AUG_ROTATE;
                op.a = engine_float(minus_engine) < 0.5f ? -angle : angle;
            }  // (an unknown name keeps kind 0: cnn_augment_matrix rejects it)
            chosen.push_back(op);
        }
        if (cnn_augment_matrix(chosen.data(), (int)chosen.size(), Hs, Ws, H, W, m) != 0) {
            std::fprintf(stderr, "ImageAugmentor::make_matrix: %s\n", cnn_amd_last_error());
            std::abort();
        }
    }

    float crop_min = 0.7f;    // the smallest crop ratio
    float max_angle = 15.f;   // degrees

private:
    static float engine_float(std::default_random_engine& e) { return std::uniform_real_distribution<float>(0.f, 1.f)(e); }
    std::vector<std::pair<std::string, float> > ops;
    std::default_random_engine engine, crop_engine, rotate_engine, minus_engine;
};

}  // namespace architectures

#endif
