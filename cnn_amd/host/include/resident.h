// resident.h -- the reference's DataLoader (cpu/include/pipeline.h, pipeline.cpp:112-140) for a dataset that lives on the device: where
// the reference decodes and resizes every image again every epoch and uploads every batch, a ResidentDataset takes the decoded bytes ONCE
// (cnn_dataset_create_u8 / _write, include/cnn_amd.h) and a ResidentLoader gathers every batch out of it by index on the device
// (cnn_batch_stager_create_u8_resident): what a batch costs on PCIe is B indices and B * 26 floats.  The loader's stager is a photo
// stager: ImageAugmentor::make_matrix and PhotoAugmentor::make_photo (augment.h) fill its per-sample maps and blocks as they do for the
// host-fed kinds, and the bits are the same.  Header only, over the C ABI alone; errors from the C ABI abort, like the reference's asserts.
#ifndef CNN_AMD_RESIDENT_H
#define CNN_AMD_RESIDENT_H

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" {
#include "cnn_amd.h"
}

using data_type = float;  // as data_format.h has it (an alias may be declared again: this header needs nothing else of that one)

namespace architectures {

// N images of Hs x Ws x 3 interleaved bytes (cv::Mat CV_8UC3 as it lies) and N labels in device memory, on the device that is current
// at construction.  Every byte starts as 0 and every label as -1.  Not copyable; destroy the loaders on it first.
// levels > 1 (up to max_levels(Hs, Ws)): each image keeps levels - 1 prefiltered half-size copies beside it, rebuilt by write(); a loader
// on the dataset then gathers every sample from the level whose residual shrink is below 2, so a map that shrinks by 2 or more no
// longer aliases.  At most a third more memory; nothing else about the loader changes.
class ResidentDataset {
public:
    ResidentDataset(const long long N, const int Hs, const int Ws, const int levels = 1) {
        must(cnn_dataset_create_u8_levels(&handle, N, Hs, Ws, levels), "ResidentDataset");
    }
    ~ResidentDataset() {
        if (handle && cnn_dataset_destroy(handle) != 0) std::fprintf(stderr, "~ResidentDataset: %s\n", cnn_amd_last_error());
    }
    ResidentDataset(const ResidentDataset&) = delete;
    ResidentDataset& operator=(const ResidentDataset&) = delete;

    // samples [first, first + count) from host memory (pageable is fine); either pointer may be null, that part is left alone.  Blocks;
    // waits first for every gather already submitted by a loader on this dataset, so a batch in flight keeps the bytes it was submitted on
    void write(const long long first, const long long count, const unsigned char* images, const int* labels) {
        must(cnn_dataset_write(handle, first, count, images, labels), "ResidentDataset::write");
    }
    // the same range back to the host; either pointer may be null.  Blocks
    void read(const long long first, const long long count, unsigned char* images, int* labels) const {
        must(cnn_dataset_read(handle, first, count, images, labels), "ResidentDataset::read");
    }
    void info(long long* N, int* Hs, int* Ws) const { must(cnn_dataset_info(handle, N, Hs, Ws), "ResidentDataset::info"); }
    static int max_levels(const int Hs, const int Ws) { return cnn_dataset_max_levels(Hs, Ws); }
    int levels() const {
        int n = 0;
        must(cnn_dataset_level_info(handle, &n, 0, nullptr, nullptr), "ResidentDataset::levels");
        return n;
    }
    void level_size(const int level, int* H_l, int* W_l) const { must(cnn_dataset_level_info(handle, nullptr, level, H_l, W_l), "ResidentDataset::level_size"); }
    // one level of the same range back to the host, [count][H_l][W_l][3].  Blocks
    void read_level(const int level, const long long first, const long long count, unsigned char* images) const {
        must(cnn_dataset_read_level(handle, level, first, count, images), "ResidentDataset::read_level");
    }
    long long size() const {
        long long n = 0;
        info(&n, nullptr, nullptr);
        return n;
    }
    void* get() const { return handle; }

    static void must(const int rc, const char* what) {
        if (rc != 0) {
            std::fprintf(stderr, "%s: %s\n", what, cnn_amd_last_error());
            std::abort();
        }
    }

private:
    void* handle = nullptr;
};

// One stager on a dataset: B samples per batch, gathered, resized to H x W, augmented and converted on the stager's own stream while the
// consumer's stream trains on the batch before.
//   next(indices, matrices, photo)  takes the next free slot (blocks on the host until its previous consumer is done), copies the B
//        indices (each in [-1, N); -1: no sample -- a fill image with label -1, for the padded tail of an evaluation pass; a training step
//        must not see one, its loss head indexes the row by the label), the B * 6 map floats and the B * 20 photo floats (null: what
//        acquire() presets -- the plain resize, no jitter, no box) and submits: one upload, one launch
//   done(slot, stream)              the consumer on `stream` has been enqueued: the slot may be reused once `stream` gets there
// Between the two the caller makes its stream wait: wait(slot, stream) (enqueue only), then reads Batch::batch and Batch::labels_dev.
// set_normalize / set_fill: the stager's, for later batches.
class ResidentLoader {
public:
    struct Batch {
        data_type* batch;  // device fp32 [B][3][H][W]
        const int* labels_dev;      // device int32 [B]: labels[idx], -1 where idx is -1
        int slot;
    };

    ResidentLoader(const ResidentDataset& dataset, const int _B, const int H, const int W, const int depth = 2) : B(_B) {
        ResidentDataset::must(cnn_batch_stager_create_u8_resident(&stager, dataset.get(), B, H, W, depth), "ResidentLoader");
    }
    ~ResidentLoader() {
        if (stager) cnn_batch_stager_destroy(stager);
    }
    ResidentLoader(const ResidentLoader&) = delete;
    ResidentLoader& operator=(const ResidentLoader&) = delete;

    void set_normalize(const float mean[3], const float std[3], const bool clamp) {
        ResidentDataset::must(cnn_batch_stager_set_normalize(stager, mean, std, clamp ? 1 : 0), "ResidentLoader::set_normalize");
    }
    void set_fill(const float fill) { ResidentDataset::must(cnn_batch_stager_set_fill(stager, fill), "ResidentLoader::set_fill"); }

    Batch next(const int* indices, const float* matrices = nullptr, const float* photo = nullptr) {
        void* host = nullptr;  // (null for this kind: the images are in the dataset)
        void* dev = nullptr;
        int* idx = nullptr;
        float* m = nullptr;
        float* p = nullptr;
        const int* labels = nullptr;
        Batch out = {nullptr, nullptr, -1};
        ResidentDataset::must(cnn_batch_stager_acquire(stager, &host, &out.slot), "ResidentLoader::next (acquire)");
        ResidentDataset::must(cnn_batch_stager_indices(stager, out.slot, &idx), "ResidentLoader::next (indices)");
        std::memcpy(idx, indices, sizeof(int) * (size_t)B);
        if (matrices) {
            ResidentDataset::must(cnn_batch_stager_matrices(stager, out.slot, &m), "ResidentLoader::next (matrices)");
            std::memcpy(m, matrices, sizeof(float) * 6 * (size_t)B);
        }
        if (photo) {
            ResidentDataset::must(cnn_batch_stager_photo(stager, out.slot, &p), "ResidentLoader::next (photo)");
            std::memcpy(p, photo, sizeof(float) * 20 * (size_t)B);
        }
        ResidentDataset::must(cnn_batch_stager_submit(stager, out.slot, &dev), "ResidentLoader::next (submit)");
        ResidentDataset::must(cnn_batch_stager_labels(stager, out.slot, &labels), "ResidentLoader::next (labels)");
        out.batch = static_cast<data_type*>(dev);
        out.labels_dev = labels;
        return out;
    }
    void wait(const int slot, void* stream) { ResidentDataset::must(cnn_batch_stager_wait(stager, slot, stream), "ResidentLoader::wait"); }
    void done(const int slot, void* stream) { ResidentDataset::must(cnn_batch_stager_release(stager, slot, stream), "ResidentLoader::done"); }
    int batch_size() const { return B; }

private:
    void* stager = nullptr;
    int B = 0;
};

}  // namespace architectures

#endif
