// resident_caller.cpp -- what a reference user writes in place of the DataLoader loop (decode, resize and upload every image every epoch)
// once the decoded dataset fits the card: architectures::ResidentDataset takes the bytes once, architectures::ResidentLoader gathers every
// batch by index on the device (cnn_amd/host/include/resident.h).  One epoch of Sequential::train_step with one batch of
// look-ahead, then a validation pass through eval_step whose last row is padded with -1.  tests/test_resident_compile.py compiles it
// against the public headers; nothing here is run.
#include <algorithm>
#include <cstddef>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "architectures.h"
#include "augment.h"
#include "resident.h"

// decode once (the caller's cv::imread + cv::resize to Hs x Ws), upload once
void fill_dataset(architectures::ResidentDataset& dataset, const std::vector<const unsigned char*>& decoded, const std::vector<int>& labels) {
    for (size_t i = 0; i < decoded.size(); ++i) dataset.write((long long)i, 1, decoded[i], &labels[i]);
}

static std::vector<tensor> views(data_type* batch, const int B, const int H, const int W) {
    std::vector<tensor> out;
    for (int b = 0; b < B; ++b) out.emplace_back(Tensor3D::device_view(3, H, W, batch + (size_t)b * 3 * H * W, "input_" + std::to_string(b)));
    return out;
}

// one training epoch: a fresh permutation, full batches only (a -1 must not reach the training loss head), augmentation sampled per image
void train_epoch(architectures::Sequential& net, architectures::ResidentDataset& dataset, architectures::ResidentLoader& loader,
                 architectures::ImageAugmentor& geometric, architectures::PhotoAugmentor& photometric, const int Hs, const int Ws, const int H,
                 const int W, const unsigned epoch, const data_type lr) {
    const int B = loader.batch_size();
    std::vector<int> order((size_t)dataset.size());
    std::iota(order.begin(), order.end(), 0);
    std::shuffle(order.begin(), order.end(), std::default_random_engine(1234u + epoch));
    const size_t steps = order.size() / (size_t)B;  // drop_last
    std::vector<float> matrices((size_t)B * 6), photo((size_t)B * 20);
    auto submit = [&](const size_t step) {
        for (int b = 0; b < B; ++b) {
            geometric.make_matrix(Hs, Ws, H, W, matrices.data() + 6 * (size_t)b);
            photometric.make_photo(H, W, photo.data() + 20 * (size_t)b);
        }
        return loader.next(order.data() + step * (size_t)B, matrices.data(), photo.data());
    };
    if (steps == 0) return;
    architectures::ResidentLoader::Batch ahead = submit(0);
    for (size_t step = 0; step < steps; ++step) {
        const architectures::ResidentLoader::Batch now = ahead;
        if (step + 1 < steps) ahead = submit(step + 1);  // its gather runs while this batch trains
        loader.wait(now.slot, architectures::stream);
        net.train_step(views(now.batch, B, H, W), now.labels_dev, lr);
        loader.done(now.slot, architectures::stream);
    }
}

// one validation pass in the stored order; the tail of the last row is -1: fill images whose label -1 is counted as ignored
architectures::EvalResult validate(architectures::Sequential& net, architectures::ResidentDataset& dataset, architectures::ResidentLoader& loader,
                                   const int H, const int W) {
    const int B = loader.batch_size();
    const long long n = dataset.size();
    std::vector<int> row((size_t)B);
    net.eval_begin(/*top_k=*/1);
    for (long long first = 0; first < n; first += B) {
        for (int b = 0; b < B; ++b) row[(size_t)b] = first + b < n ? (int)(first + b) : -1;
        const architectures::ResidentLoader::Batch now = loader.next(row.data());  // the presets: plain resize, no jitter, no box
        loader.wait(now.slot, architectures::stream);
        net.eval_step(views(now.batch, B, H, W), now.labels_dev);
        loader.done(now.slot, architectures::stream);
    }
    return net.eval_result();  // the one synchronise
}

int run(architectures::Sequential& net, const std::vector<const unsigned char*>& decoded, const std::vector<int>& labels, const int Hs, const int Ws) {
    const int B = 64, H = 224, W = 224;
    architectures::ResidentDataset dataset((long long)decoded.size(), Hs, Ws);
    fill_dataset(dataset, decoded, labels);
    long long n = 0;
    int hs = 0, ws = 0;
    dataset.info(&n, &hs, &ws);
    std::vector<int> back(1);
    dataset.read(0, 1, nullptr, back.data());
    architectures::ResidentLoader loader(dataset, B, H, W, /*depth=*/2);
    const float mean[3] = {0.406f, 0.456f, 0.485f}, std_[3] = {0.225f, 0.224f, 0.229f};  // ImageNet's, in cv::imread's BGR order
    loader.set_normalize(mean, std_, /*clamp=*/true);
    loader.set_fill(0.f);
    architectures::ImageAugmentor geometric;
    architectures::PhotoAugmentor photometric;
    train_epoch(net, dataset, loader, geometric, photometric, hs, ws, H, W, /*epoch=*/0, 1e-3f);
    const architectures::EvalResult r = validate(net, dataset, loader, H, W);
    return (r.samples == (uint64_t)n && back[0] == labels[0]) ? 0 : 1;
}
