// augment.h -- the reference's ImageAugmentor (cpu/include/pipeline.h, pipeline.cpp:40-77) for the device path: constructed like the
// reference's, from op names and probabilities, but instead of transforming a cv::Mat on the host it SAMPLES the same decisions and
// composes them into the six floats of one output -> source map (cnn_augment_matrix, include/cnn_amd.h).  A caller fills a slot of an
// augmenting stager (cnn_batch_stager_create_u8_aug) with one such map per image; the gather itself runs on the device, fused with the
// bytes -> fp32 conversion.  Header only; errors from the C ABI abort, like the reference's asserts.
#ifndef CNN_AMD_AUGMENT_H
#define CNN_AMD_AUGMENT_H

#include <algorithm>
#include <cmath>
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

// The photometric half for a photo stager (cnn_batch_stager_create_u8_photo): constructed the same way, from op names and probabilities,
// it samples one image's colour jitter and erase box into the 20 floats of cnn_batch_stager_photo's block (include/cnn_amd.h: A[9], o[3],
// ex0, ey0, ew, eh, ev[3], 0).  The colour ops compose through cnn_colour_matrix: contrast pivots on the fixed `pivot`, hue is the linear
// YIQ rotation, nothing clamps between the ops; the kernel clamps once if the stager's normalisation says so.  One box, one value per
// channel: per-pixel noise is not covered.
class PhotoAugmentor {
public:
    // op names: "brightness", "contrast", "saturation", "hue", "erase"; second = the probability that the op fires for an image
    explicit PhotoAugmentor(const std::vector<std::pair<std::string, float> >& _ops = {{"brightness", 1.f}, {"contrast", 1.f}, {"saturation", 1.f},
                                                                                      {"erase", 0.25f}},
                            const unsigned seed = 212)
        : ops(_ops), engine(seed), colour_engine(seed + 1), erase_engine(seed + 2) {}

    // One image's block for an H x W output: the colour ops in a shuffled order (ColorJitter's sampling: factors uniform in
    // [max(0, 1 - a), 1 + a], hue uniform in [-hue, hue] degrees); "erase": timm's RandomErasing sampling -- up to 10 attempts of an
    // area fraction uniform in [area_min, area_max] and an aspect ratio log-uniform in [aspect_min, aspect_max], the first box that
    // fits (1 <= w < W, 1 <= h < H) at a uniform position; its value is 0 (output units), or one normal value per channel (erase_rand).
    void make_photo(const int H, const int W, float p[20]) {
        std::shuffle(ops.begin(), ops.end(), engine);
        std::vector<cnn_colour_op> chosen;
        for (int i = 12; i < 20; ++i) p[i] = 0.f;
        for (const auto& item : ops) {
            if (!(unit(engine) < item.second)) continue;
            cnn_colour_op op = {0, 0.f, 0.f};
            if (item.first == "erase") {
                make_box(H, W, p);
                continue;
            }
            if (item.first == "brightness") { op.kind = CNN_COL_BRIGHTNESS; op.a = factor(brightness); }
            else if (item.first == "contrast") { op.kind = CNN_COL_CONTRAST; op.a = factor(contrast); op.b = pivot; }
            else if (item.first == "saturation") { op.kind = CNN_COL_SATURATION; op.a = factor(saturation); }
            else if (item.first == "hue") { op.kind = CNN_COL_HUE; op.a = hue * (2.f * unit(colour_engine) - 1.f); }
            // (an unknown name keeps kind 0: cnn_colour_matrix rejects it)
            chosen.push_back(op);
        }
        if (cnn_colour_matrix(chosen.data(), (int)chosen.size(), p) != 0) {
            std::fprintf(stderr, "PhotoAugmentor::make_photo: %s\n", cnn_amd_last_error());
            std::abort();
        }
    }

    float brightness = 0.4f, contrast = 0.4f, saturation = 0.4f;  // amplitudes a: factors in [max(0, 1 - a), 1 + a]
    float hue = 0.f;                                               // degrees
    float pivot = 0.5f;                                            // what contrast scales about
    float area_min = 0.02f, area_max = 1.f / 3.f, aspect_min = 0.3f, aspect_max = 3.3f;
    bool erase_rand = false;

private:
    static float unit(std::default_random_engine& e) { return std::uniform_real_distribution<float>(0.f, 1.f)(e); }
    float factor(const float a) {
        const float lo = std::max(0.f, 1.f - a);
        return lo + (1.f + a - lo) * unit(colour_engine);
    }
    void make_box(const int H, const int W, float p[20]) {
        for (int attempt = 0; attempt < 10; ++attempt) {
            const float target = (area_min + (area_max - area_min) * unit(erase_engine)) * (float)H * (float)W;
            const float la = std::log(aspect_min) + (std::log(aspect_max) - std::log(aspect_min)) * unit(erase_engine);
            const float aspect = std::exp(la);
            const int h = (int)std::lround(std::sqrt(target * aspect)), w = (int)std::lround(std::sqrt(target / aspect));
            if (!(w >= 1 && w < W && h >= 1 && h < H)) continue;
            p[12] = (float)std::uniform_int_distribution<int>(0, W - w)(erase_engine);
            p[13] = (float)std::uniform_int_distribution<int>(0, H - h)(erase_engine);
            p[14] = (float)w;
            p[15] = (float)h;
            if (erase_rand)
                for (int c = 0; c < 3; ++c) p[16 + c] = std::normal_distribution<float>(0.f, 1.f)(erase_engine);
            return;
        }
    }
    std::vector<std::pair<std::string, float> > ops;
    std::default_random_engine engine, colour_engine, erase_engine;
};

}  // namespace architectures

#endif
