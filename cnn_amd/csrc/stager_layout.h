// stager_layout.h -- what kind a batch stager is and what one of its slots holds, stated once (staging.hip allocates, hands out and
// uploads by it; augment.hip shares the limits).  Plain C++17: no HIP, no common.h, so tests/caller/stager_layout_check.cpp holds it to
// include/cnn_amd.h on the CPU under the sanitizers.
#pragma once
#include <cstddef>

namespace cnn_amd {

constexpr int kMaxDim = 8192;    // B and every image dimension: fp32 holds every pixel index (and index + 0.5) below this exactly
constexpr int kMaxLevels = 14;   // 8192 halves to 1 in 13 steps
constexpr int kMapFloats = 6;    // a sample's map (and its level map)
constexpr int kPhotoFloats = 20; // a sample's photo block

// include/cnn_amd.h: cnn_batch_stager_create, _create_u8, _create_u8_aug, _create_u8_photo, _create_u8_resident
enum class StagerKind { Raw, U8, Aug, Photo, Resident };

struct StagerShape {
    StagerKind kind = StagerKind::Raw;
    int B = 0, Hs = 0, Ws = 0, H = 0, W = 0;  // U8: Hs x Ws is H x W; Resident: the dataset's level 0
    int levels = 1;                           // Resident: the dataset's
    size_t batch_bytes = 0;                   // Raw only
};

// the parts of a slot's parameter block, in the order they lie in it; each is B * stager_part_words() 4-byte words (int32 or float)
enum class StagerPart { Indices, Maps, Photo, Levels, LevelMaps };
constexpr int kStagerParts = 5;
constexpr size_t stager_part_words(StagerPart p) {
    return p == StagerPart::Photo ? kPhotoFloats : (p == StagerPart::Maps || p == StagerPart::LevelMaps) ? kMapFloats : 1;
}

// which parts a stager has -- and so which accessors answer: _matrices and _set_fill with Maps, _photo and _set_normalize with Photo,
// _indices and _labels with Indices, _levels with Levels
constexpr bool stager_has(const StagerShape& s, StagerPart p) {
    switch (p) {
    case StagerPart::Maps: return s.kind == StagerKind::Aug || s.kind == StagerKind::Photo || s.kind == StagerKind::Resident;
    case StagerPart::Photo: return s.kind == StagerKind::Photo || s.kind == StagerKind::Resident;
    case StagerPart::Indices: return s.kind == StagerKind::Resident;
    default: return s.kind == StagerKind::Resident && s.levels > 1;  // Levels, LevelMaps
    }
}

constexpr size_t kNoPart = ~(size_t)0;
struct SlotLayout {
    size_t image_bytes = 0;  // the pinned image block and its device copy (Resident: none, the images are the dataset's)
    size_t param_bytes = 0;  // the pinned parameter block and its device copy: ONE allocation and one upload each (Raw, U8: none)
    size_t offset[kStagerParts] = {kNoPart, kNoPart, kNoPart, kNoPart, kNoPart};  // of each part inside that block, by StagerPart
    size_t out_bytes = 0;    // the fp32 [B][3][H][W] batch submit() hands out (Raw: none, it hands out the image block's device copy)
    size_t label_bytes = 0;  // the gathered labels, device int32 [B] (Resident only)
};
constexpr SlotLayout slot_layout(const StagerShape& s) {
    SlotLayout l;
    const size_t B = (size_t)s.B;
    l.image_bytes = s.kind == StagerKind::Raw ? s.batch_bytes : s.kind == StagerKind::Resident ? 0 : B * (size_t)s.Hs * (size_t)s.Ws * 3;
    for (int p = 0; p < kStagerParts; ++p)
        if (stager_has(s, (StagerPart)p)) {
            l.offset[p] = l.param_bytes;
            l.param_bytes += B * stager_part_words((StagerPart)p) * 4;
        }
    l.out_bytes = s.kind == StagerKind::Raw ? 0 : B * 3 * (size_t)s.H * (size_t)s.W * sizeof(float);
    l.label_bytes = s.kind == StagerKind::Resident ? B * sizeof(int) : 0;
    return l;
}

}  // namespace cnn_amd
