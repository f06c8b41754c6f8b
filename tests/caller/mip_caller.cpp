// mip_caller.cpp -- what a reference user writes to keep photos near their native size on the card and let the loader's map do the resize:
// an architectures::ResidentDataset with half-size levels (cnn_amd/host/include/resident.h).  The loader, the training
// loop and the validation pass are those of tests/caller/resident_caller.cpp, unchanged: levels are a property of the dataset.
// tests/test_mip_compile.py compiles it against the public headers; nothing here is run.
#include <algorithm>
#include <cstddef>
#include <vector>

#include "resident.h"

// 512 x 512 photos for a 224 x 224 net: a random-resized crop may shrink by up to 512 / 224 and more, so two half-size levels
int run(const std::vector<const unsigned char*>& decoded, const std::vector<int>& labels) {
    const int Hs = 512, Ws = 512, B = 64, H = 224, W = 224;
    const int levels = std::min(3, architectures::ResidentDataset::max_levels(Hs, Ws));
    architectures::ResidentDataset dataset((long long)decoded.size(), Hs, Ws, levels);
    architectures::ResidentDataset plain((long long)decoded.size(), Hs, Ws);  // one level: what it always was
    for (size_t i = 0; i < decoded.size(); ++i) dataset.write((long long)i, 1, decoded[i], &labels[i]);  // rebuilds the levels of sample i
    if (dataset.levels() != levels || plain.levels() != 1) return 1;
    int h1 = 0, w1 = 0;
    dataset.level_size(1, &h1, &w1);
    std::vector<unsigned char> half((size_t)h1 * (size_t)w1 * 3);
    dataset.read_level(1, 0, 1, half.data());

    // the level a map will gather from, and its map there, can be asked for on the host
    float m[6], m_level[6];
    int level = -1;
    architectures::ResidentDataset::must(cnn_augment_matrix(nullptr, 0, Hs, Ws, H, W, m), "cnn_augment_matrix");
    architectures::ResidentDataset::must(cnn_augment_level(m, levels, &level, m_level), "cnn_augment_level");

    architectures::ResidentLoader loader(dataset, B, H, W, /*depth=*/2);
    std::vector<int> row((size_t)B, -1);
    for (int b = 0; b < B && b < (int)decoded.size(); ++b) row[(size_t)b] = b;
    const architectures::ResidentLoader::Batch now = loader.next(row.data());  // the presets: the plain resize, gathered from level 1
    loader.wait(now.slot, nullptr);
    loader.done(now.slot, nullptr);
    return (level == 1 && half.size() == (size_t)256 * 256 * 3 && now.batch != nullptr) ? 0 : 1;
}
