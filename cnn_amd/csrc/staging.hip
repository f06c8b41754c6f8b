// staging.hip -- input staging (include/cnn_amd.h, "input staging" and below): the batch stager in its five kinds and the device-resident
// uint8 dataset.  A stager owns `depth` slots, a copy stream and two events per slot; what a slot of each kind holds, and where the parts
// of its parameter block lie, is stager_layout.h's to say -- create, the accessors, acquire, submit and destroy all go by it.  The
// augmenting kinds launch augment.hip's kernel (augment_u8_run), the u8 kind the plain conversion below.
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"

using namespace cnn_amd;

namespace {
struct Dataset;

struct Slot {
    void *img_host = nullptr, *img_dev = nullptr;  // the image block (pinned) and its device copy
    char *par_host = nullptr, *par_dev = nullptr;  // the parameter block (pinned) and its device copy
    void* out = nullptr;                           // the fp32 batch submit() hands out
    int* labels = nullptr;                         // device: the labels the resident kernel gathers beside the batch
    hipEvent_t uploaded = nullptr, consumed = nullptr;
    bool in_use = false;  // `consumed` has been recorded at least once
};
struct Stager {
    StagerShape shape;
    SlotLayout lay;
    std::vector<Slot> slots;
    int next = 0;
    hipStream_t copy = nullptr;
    float fill = 0.f;
    float resize_map[6] = {1, 0, 0, 0, 1, 0};     // what acquire() presets: the plain resize of the source to W x H
    PhotoNorm norm = {{1.f, 1.f, 1.f}, {0.f, 0.f, 0.f}, 0};  // the normalisation of later submits (cnn_batch_stager_set_normalize)
    Dataset* ds = nullptr;                         // Resident: the source
    int depth() const { return (int)slots.size(); }
    bool has(StagerPart p) const { return stager_has(shape, p); }
    template <class T>
    T* host_part(const Slot& s, StagerPart p) const { return reinterpret_cast<T*>(s.par_host + lay.offset[(int)p]); }
    template <class T>
    T* dev_part(const Slot& s, StagerPart p) const { return reinterpret_cast<T*>(s.par_dev + lay.offset[(int)p]); }
};

// cnn_dataset_create_u8: N images of Hs x Ws x 3 bytes and N labels on `device`; `stagers` (under `mu`): the resident stagers attached.
// cnn_dataset_create_u8_levels: `level` has one row per level (level[0].base == 0: the level-0 region keeps the one-level layout, the
// higher levels follow it in the same allocation); with more than one level `table` is its device copy and `stream` the stream the
// rebuild kernels of write() run on -- both stay null for a one-level dataset, which is what it always was
struct Dataset {
    long long N = 0;
    int Hs = 0, Ws = 0, device = 0;
    size_t sample_bytes = 0;
    unsigned char* images = nullptr;
    int* labels = nullptr;
    std::vector<DatasetLevel> level;
    DatasetLevel* table = nullptr;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::vector<Stager*> stagers;
};
}  // namespace

extern "C" {  // (the two kernels' symbols in the code object are their plain names)
namespace {
// Tensor3D::read_from_opencv_mat (data_format.cpp:13-23) for a whole batch: interleaved bytes [B][H*W][3] -> planar fp32 [B][3][H*W].
// A thread converts four consecutive pixels: 12 bytes in (three 4-byte loads), one 16-byte store into each channel plane.  The table
// lives in LDS (no arithmetic on the device: the host's v * 1.f / 255, bit for bit).
__global__ __launch_bounds__(256) void u8hwc_to_f32chw(const unsigned* __restrict__ src, float* __restrict__ dst, const float* __restrict__ lut_g,
                                                       int hw4, long long quads_total) {
    __shared__ float lut[256];
    lut[threadIdx.x] = lut_g[threadIdx.x];
    __syncthreads();
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads_total; q += (long long)gridDim.x * 256) {
        const long long b = q / hw4;
        const int i4 = (int)(q - b * hw4);  // quad index inside the image
        const unsigned w0 = src[3 * q], w1 = src[3 * q + 1], w2 = src[3 * q + 2];  // bytes p0c0 p0c1 p0c2 p1c0 | p1c1 p1c2 p2c0 p2c1 | p2c2 p3c0 p3c1 p3c2
        float4 c0, c1, c2;
        c0.x = lut[w0 & 255u];         c1.x = lut[(w0 >> 8) & 255u];  c2.x = lut[(w0 >> 16) & 255u];
        c0.y = lut[w0 >> 24];          c1.y = lut[w1 & 255u];         c2.y = lut[(w1 >> 8) & 255u];
        c0.z = lut[(w1 >> 16) & 255u]; c1.z = lut[w1 >> 24];          c2.z = lut[w2 & 255u];
        c0.w = lut[(w2 >> 8) & 255u];  c1.w = lut[(w2 >> 16) & 255u]; c2.w = lut[w2 >> 24];
        float* d = dst + (size_t)b * 12 * hw4 + 4 * (size_t)i4;  // image b, channel 0, pixel 4*i4
        *(float4*)d = c0;
        *(float4*)(d + 4 * (size_t)hw4) = c1;
        *(float4*)(d + 8 * (size_t)hw4) = c2;
    }
}
// ... and for images whose pixel count is no multiple of four (round 6: any H, W): one thread per pixel, three byte loads, three stores
__global__ __launch_bounds__(256) void u8hwc_to_f32chw_px(const unsigned char* __restrict__ src, float* __restrict__ dst, const float* __restrict__ lut_g,
                                                          int hw, long long px_total) {
    __shared__ float lut[256];
    lut[threadIdx.x] = lut_g[threadIdx.x];
    __syncthreads();
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < px_total; q += (long long)gridDim.x * 256) {
        const long long b = q / hw;
        const int i = (int)(q - b * hw);
        float* d = dst + (size_t)b * 3 * hw + i;
        d[0] = lut[src[3 * q]];
        d[(size_t)hw] = lut[src[3 * q + 1]];
        d[2 * (size_t)hw] = lut[src[3 * q + 2]];
    }
}
}  // namespace
}  // extern "C"

namespace {
// what a sample's photo block is preset to: A = I, o = 0, no box -- with s = 1, t = 0, clamp off the gather rule's bits unchanged
const float kPhotoIdentity[kPhotoFloats] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// The one create behind the five entry points, which have checked their arguments: `depth` slots of what the layout says.  *stager is set
// before the first allocation, so that a caller can destroy a partially built stager after a failed create (destroy frees what is there).
int stager_create(void** stager, const StagerShape& shape, int depth, const float* resize_map = nullptr, Dataset* ds = nullptr) {
    Stager* st = new Stager();
    st->shape = shape;
    st->lay = slot_layout(shape);
    st->slots.resize((size_t)depth);
    st->ds = ds;
    if (resize_map) memcpy(st->resize_map, resize_map, sizeof(st->resize_map));
    *stager = st;
    const SlotLayout& lay = st->lay;
    CNN_HIP_CHECK(hipStreamCreateWithFlags(&st->copy, hipStreamNonBlocking));
    if (lay.out_bytes) {  // every kind that launches reads the byte -> float table: made here, so that no submit pays for its upload
        const float* lut = nullptr;
        if (int rc = device_lut(&lut)) return rc;
    }
    for (Slot& s : st->slots) {
        if (lay.image_bytes) {
            CNN_HIP_CHECK(hipHostMalloc(&s.img_host, lay.image_bytes, hipHostMallocDefault));
            CNN_HIP_CHECK(hipMalloc(&s.img_dev, lay.image_bytes));
        }
        if (lay.param_bytes) {
            CNN_HIP_CHECK(hipHostMalloc((void**)&s.par_host, lay.param_bytes, hipHostMallocDefault));
            CNN_HIP_CHECK(hipMalloc((void**)&s.par_dev, lay.param_bytes));
            memset(s.par_host, 0, lay.param_bytes);  // (the levels read as 0 before the first submit)
        }
        if (lay.out_bytes) CNN_HIP_CHECK(hipMalloc(&s.out, lay.out_bytes));
        if (lay.label_bytes) CNN_HIP_CHECK(hipMalloc((void**)&s.labels, lay.label_bytes));
        CNN_HIP_CHECK(hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming));
        CNN_HIP_CHECK(hipEventCreateWithFlags(&s.consumed, hipEventDisableTiming));
    }
    if (ds) {
        std::lock_guard<std::mutex> lk(ds->mu);
        ds->stagers.push_back(st);
    }
    return CNN_AMD_OK;
}

// what an accessor says on a stager without its part
const char* const kLacks[kStagerParts] = {
    "not a resident stager (cnn_batch_stager_create_u8_resident)", "not an augmenting stager (cnn_batch_stager_create_u8_aug)",
    "not a photo stager (cnn_batch_stager_create_u8_photo)", "the stager's dataset has one level (cnn_dataset_create_u8_levels)",
    "the stager's dataset has one level (cnn_dataset_create_u8_levels)"};
int require_part(const char* who, const Stager* st, StagerPart part) {
    if (part == StagerPart::Levels) CNN_REQUIRE(st->has(StagerPart::Indices), "%s: %s", who, kLacks[(int)StagerPart::Indices]);
    CNN_REQUIRE(st->has(part), "%s: %s", who, kLacks[(int)part]);
    return CNN_AMD_OK;
}
// a slot's pinned part, for the caller to write (the levels: to read)
template <class T>
int slot_part(const char* who, void* stager, int slot, StagerPart part, T** pinned) {
    Stager* st = static_cast<Stager*>(stager);
    CNN_REQUIRE(st && pinned && slot >= 0 && slot < st->depth(), "%s: bad arguments", who);
    if (int rc = require_part(who, st, part)) return rc;
    *pinned = st->host_part<T>(st->slots[(size_t)slot], part);
    return CNN_AMD_OK;
}
}  // namespace

extern "C" {

int cnn_batch_stager_create(void** stager, size_t batch_bytes, int depth) {
    CNN_REQUIRE(stager && batch_bytes > 0 && depth >= 2 && depth <= 16, "cnn_batch_stager_create: bad arguments (depth 2..16)");
    StagerShape shape;
    shape.batch_bytes = batch_bytes;
    return stager_create(stager, shape, depth);
}

int cnn_batch_stager_create_u8(void** stager, int B, int H, int W, int depth) {
    CNN_REQUIRE(stager && B > 0 && H > 0 && W > 0 && depth >= 2 && depth <= 16, "cnn_batch_stager_create_u8: bad arguments (depth 2..16)");
    StagerShape shape;
    shape.kind = StagerKind::U8;
    shape.B = B; shape.Hs = shape.H = H; shape.Ws = shape.W = W;
    return stager_create(stager, shape, depth);
}

namespace {
int create_u8_aug(void** stager, StagerKind kind, int B, int Hs, int Ws, int H, int W, int depth, Dataset* ds = nullptr) {
    float map[6];
    if (int rc = cnn_augment_matrix(nullptr, 0, Hs, Ws, H, W, map)) return rc;  // (checks the four dimensions)
    StagerShape shape;
    shape.kind = kind;
    shape.B = B; shape.Hs = Hs; shape.Ws = Ws; shape.H = H; shape.W = W;
    if (ds) shape.levels = (int)ds->level.size();
    return stager_create(stager, shape, depth, map, ds);
}
}  // namespace

int cnn_batch_stager_create_u8_aug(void** stager, int B, int Hs, int Ws, int H, int W, int depth) {
    CNN_REQUIRE(stager && B > 0 && B <= kMaxDim && depth >= 2 && depth <= 16, "cnn_batch_stager_create_u8_aug: bad arguments (B 1..8192, depth 2..16)");
    return create_u8_aug(stager, StagerKind::Aug, B, Hs, Ws, H, W, depth);
}

int cnn_batch_stager_create_u8_photo(void** stager, int B, int Hs, int Ws, int H, int W, int depth) {
    CNN_REQUIRE(stager && B > 0 && B <= kMaxDim && depth >= 2 && depth <= 16, "cnn_batch_stager_create_u8_photo: bad arguments (B 1..8192, depth 2..16)");
    return create_u8_aug(stager, StagerKind::Photo, B, Hs, Ws, H, W, depth);
}

int cnn_batch_stager_create_u8_resident(void** stager, void* dataset, int B, int H, int W, int depth) {
    Dataset* ds = static_cast<Dataset*>(dataset);
    CNN_REQUIRE(stager && ds && B > 0 && B <= kMaxDim && depth >= 2 && depth <= 16,
                "cnn_batch_stager_create_u8_resident: bad arguments (a dataset, B 1..8192, depth 2..16)");
    int dev = 0;
    CNN_HIP_CHECK(hipGetDevice(&dev));
    CNN_REQUIRE(dev == ds->device, "cnn_batch_stager_create_u8_resident: the dataset lives on device %d, the current device is %d", ds->device, dev);
    return create_u8_aug(stager, StagerKind::Resident, B, ds->Hs, ds->Ws, H, W, depth, ds);
}

int cnn_batch_stager_matrices(void* stager, int slot, float** pinned) { return slot_part("cnn_batch_stager_matrices", stager, slot, StagerPart::Maps, pinned); }
int cnn_batch_stager_photo(void* stager, int slot, float** pinned) { return slot_part("cnn_batch_stager_photo", stager, slot, StagerPart::Photo, pinned); }
int cnn_batch_stager_indices(void* stager, int slot, int** pinned) { return slot_part("cnn_batch_stager_indices", stager, slot, StagerPart::Indices, pinned); }
int cnn_batch_stager_levels(void* stager, int slot, const int** pinned) { return slot_part("cnn_batch_stager_levels", stager, slot, StagerPart::Levels, pinned); }

int cnn_batch_stager_labels(void* stager, int slot, const int** labels_dev) {
    Stager* st = static_cast<Stager*>(stager);
    CNN_REQUIRE(st && labels_dev && slot >= 0 && slot < st->depth(), "cnn_batch_stager_labels: bad arguments");
    if (int rc = require_part("cnn_batch_stager_labels", st, StagerPart::Indices)) return rc;
    *labels_dev = st->slots[(size_t)slot].labels;
    return CNN_AMD_OK;
}

int cnn_batch_stager_set_fill(void* stager, float fill) {
    Stager* st = static_cast<Stager*>(stager);
    CNN_REQUIRE(st, "cnn_batch_stager_set_fill: null stager");
    if (int rc = require_part("cnn_batch_stager_set_fill", st, StagerPart::Maps)) return rc;
    CNN_REQUIRE(fill - fill == 0.f, "cnn_batch_stager_set_fill: fill is not finite");
    st->fill = fill;
    return CNN_AMD_OK;
}

int cnn_batch_stager_set_normalize(void* stager, const float mean[3], const float std[3], int clamp) {
    Stager* st = static_cast<Stager*>(stager);
    CNN_REQUIRE(st && mean && std, "cnn_batch_stager_set_normalize: null pointer");
    if (int rc = require_part("cnn_batch_stager_set_normalize", st, StagerPart::Photo)) return rc;
    PhotoNorm n;
    for (int c = 0; c < 3; ++c) {
        CNN_REQUIRE(mean[c] - mean[c] == 0.f && std[c] - std[c] == 0.f && std[c] != 0.f,
                    "cnn_batch_stager_set_normalize: channel %d: mean must be finite, std finite and non-zero", c);
        n.s[c] = (float)(1.0 / (double)std[c]);
        n.t[c] = (float)(-(double)mean[c] / (double)std[c] + 0.0);  // (+ 0.0: a mean of 0 leaves -0)
        CNN_REQUIRE(n.s[c] - n.s[c] == 0.f && n.t[c] - n.t[c] == 0.f, "cnn_batch_stager_set_normalize: channel %d: 1/std or mean/std is not finite in fp32", c);
    }
    n.clamp = clamp ? 1 : 0;
    st->norm = n;
    return CNN_AMD_OK;
}

int cnn_batch_stager_destroy(void* stager) {
    Stager* st = static_cast<Stager*>(stager);
    if (!st) return CNN_AMD_OK;
    if (st->copy) (void)hipStreamSynchronize(st->copy);
    if (st->ds) {  // detach: the dataset may be written without waiting for this stream, and destroyed
        std::lock_guard<std::mutex> lk(st->ds->mu);
        std::vector<Stager*>& v = st->ds->stagers;
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i] == st) {
                v.erase(v.begin() + (long)i);
                break;
            }
    }
    for (Slot& s : st->slots) {  // what stager_create allocated, as far as it got
        if (s.img_host) (void)hipHostFree(s.img_host);
        if (s.img_dev) (void)hipFree(s.img_dev);
        if (s.par_host) (void)hipHostFree(s.par_host);
        if (s.par_dev) (void)hipFree(s.par_dev);
        if (s.out) (void)hipFree(s.out);
        if (s.labels) (void)hipFree(s.labels);
        if (s.uploaded) (void)hipEventDestroy(s.uploaded);
        if (s.consumed) (void)hipEventDestroy(s.consumed);
    }
    if (st->copy) (void)hipStreamDestroy(st->copy);
    delete st;
    return CNN_AMD_OK;
}

int cnn_batch_stager_acquire(void* stager, void** pinned_host, int* slot) {
    Stager* st = static_cast<Stager*>(stager);
    CNN_REQUIRE(st && pinned_host && slot, "cnn_batch_stager_acquire: null pointer");
    const int i = st->next;
    st->next = (st->next + 1) % st->depth();
    Slot& s = st->slots[(size_t)i];
    // the previous upload out of this slot must have left the host buffer, and its consumer must be done with the device one
    CNN_HIP_CHECK(hipEventSynchronize(s.uploaded));
    if (s.in_use) CNN_HIP_CHECK(hipEventSynchronize(s.consumed));
    const int B = st->shape.B;
    if (st->has(StagerPart::Maps))
        for (int b = 0; b < B; ++b) memcpy(st->host_part<float>(s, StagerPart::Maps) + kMapFloats * (size_t)b, st->resize_map, sizeof(st->resize_map));
    if (st->has(StagerPart::Photo))
        for (int b = 0; b < B; ++b) memcpy(st->host_part<float>(s, StagerPart::Photo) + kPhotoFloats * (size_t)b, kPhotoIdentity, sizeof(kPhotoIdentity));
    if (st->has(StagerPart::Indices))
        for (int b = 0; b < B; ++b) st->host_part<int>(s, StagerPart::Indices)[b] = -1;
    *pinned_host = s.img_host;  // (null for a resident stager: its images are in the dataset)
    *slot = i;
    return CNN_AMD_OK;
}

namespace {
// the slot's one launch, behind its copies on the copy stream: none (Raw), the plain conversion (U8), the augmenting gather (the rest)
int stager_launch(const Stager* st, const Slot& s) {
    const StagerShape& sh = st->shape;
    if (sh.kind == StagerKind::Raw) return CNN_AMD_OK;
    if (sh.kind == StagerKind::U8) {  // bytes -> the fp32 planar batch
        const float* lut = nullptr;
        if (int rc = device_lut(&lut)) return rc;
        const int hw = sh.H * sh.W;
        const bool timed = ktimer_active();  // (cnn_amd_kernel_timing_enable: tools/augment_bench.py times this launch)
        if (timed) ktimer_begin(st->copy, "u8hwc_to_f32chw", "B=%d hw=%d", sh.B, hw);
        if (hw % 4 == 0) {
            const int hw4 = hw / 4;
            const long long quads = (long long)sh.B * hw4;
            u8hwc_to_f32chw<<<stream_grid((size_t)quads, 256), 256, 0, st->copy>>>((const unsigned*)s.img_dev, (float*)s.out, lut, hw4, quads);
        } else {
            const long long px = (long long)sh.B * hw;
            u8hwc_to_f32chw_px<<<stream_grid((size_t)px, 256), 256, 0, st->copy>>>((const unsigned char*)s.img_dev, (float*)s.out, lut, hw, px);
        }
        if (timed) ktimer_end(st->copy);
        CNN_LAUNCH_CHECK();
        return CNN_AMD_OK;
    }
    // bytes (or the dataset's store) + the slot's parameter block -> the fp32 planar batch
    const char* who = sh.kind == StagerKind::Aug ? "cnn_augment_u8" : "augment_u8_photo";
    AugmentJob j = {(const unsigned char*)s.img_dev, sh.B, sh.Hs, sh.Ws, st->dev_part<const float>(s, StagerPart::Maps), st->fill, (float*)s.out, sh.H, sh.W,
                    st->has(StagerPart::Photo) ? st->dev_part<const float>(s, StagerPart::Photo) : nullptr, st->norm, ResidentArgs()};
    if (const Dataset* ds = st->ds) {
        who = "augment_u8_resident";
        j.src = ds->images;
        j.res.indices = st->dev_part<const int>(s, StagerPart::Indices);
        j.res.labels = ds->labels;
        j.res.labels_out = s.labels;
        j.res.N = ds->N;
        if (st->has(StagerPart::Levels)) {  // the kernel reads the level maps in place of the caller's
            who = "augment_u8_resident_levels";
            j.mats = st->dev_part<const float>(s, StagerPart::LevelMaps);
            j.res.levels = st->dev_part<const int>(s, StagerPart::Levels);
            j.res.table = ds->table;
            j.res.L = sh.levels;
        }
    }
    return augment_u8_run(who, j, st->copy);
}
}  // namespace

// One sequence on the copy stream for every kind: wait for the slot's consumer, copy the image block, copy the parameter block (one copy),
// launch, record `uploaded`.
int cnn_batch_stager_submit(void* stager, int slot, void** device_ptr) {
    Stager* st = static_cast<Stager*>(stager);
    CNN_REQUIRE(st && device_ptr && slot >= 0 && slot < st->depth(), "cnn_batch_stager_submit: bad arguments");
    Slot& s = st->slots[(size_t)slot];
    const SlotLayout& lay = st->lay;
    std::unique_lock<std::mutex> lk;
    if (Dataset* ds = st->ds) {
        const int B = st->shape.B;
        const int* idx = st->host_part<int>(s, StagerPart::Indices);
        for (int b = 0; b < B; ++b)  // pinned memory the caller wrote: checked before anything is enqueued
            CNN_REQUIRE(idx[b] >= -1 && (long long)idx[b] < ds->N, "cnn_batch_stager_submit: index %d of sample %d is outside [-1, %lld)", idx[b], b, ds->N);
        if (st->has(StagerPart::Levels))  // each sample's level and its map on that level, beside the caller's maps (those stay as they are)
            for (int b = 0; b < B; ++b)
                if (int rc = cnn_augment_level(st->host_part<float>(s, StagerPart::Maps) + kMapFloats * (size_t)b, st->shape.levels,
                                               st->host_part<int>(s, StagerPart::Levels) + b,
                                               st->host_part<float>(s, StagerPart::LevelMaps) + kMapFloats * (size_t)b))
                    return rc;
        lk = std::unique_lock<std::mutex>(ds->mu);  // (cnn_dataset_write drains this stream under the same lock)
    }
    if (s.in_use) CNN_HIP_CHECK(hipStreamWaitEvent(st->copy, s.consumed, 0));
    if (lay.image_bytes) CNN_HIP_CHECK(hipMemcpyAsync(s.img_dev, s.img_host, lay.image_bytes, hipMemcpyHostToDevice, st->copy));
    if (lay.param_bytes) CNN_HIP_CHECK(hipMemcpyAsync(s.par_dev, s.par_host, lay.param_bytes, hipMemcpyHostToDevice, st->copy));
    if (int rc = stager_launch(st, s)) return rc;
    CNN_HIP_CHECK(hipEventRecord(s.uploaded, st->copy));
    *device_ptr = lay.out_bytes ? s.out : s.img_dev;
    return CNN_AMD_OK;
}

int cnn_batch_stager_wait(void* stager, int slot, void* stream) {
    Stager* st = static_cast<Stager*>(stager);
    CNN_REQUIRE(st && slot >= 0 && slot < st->depth(), "cnn_batch_stager_wait: bad arguments");
    CNN_HIP_CHECK(hipStreamWaitEvent(as_stream(stream), st->slots[(size_t)slot].uploaded, 0));
    publish_mark_stale(as_stream(stream));
    return CNN_AMD_OK;
}

int cnn_batch_stager_release(void* stager, int slot, void* stream) {
    Stager* st = static_cast<Stager*>(stager);
    CNN_REQUIRE(st && slot >= 0 && slot < st->depth(), "cnn_batch_stager_release: bad arguments");
    Slot& s = st->slots[(size_t)slot];
    CNN_HIP_CHECK(hipEventRecord(s.consumed, as_stream(stream)));
    s.in_use = true;
    return CNN_AMD_OK;
}

// ---- the device-resident dataset ----------------------------------------------------------------------------------------------
namespace {
int dataset_create(const char* who, void** dataset, long long N, int Hs, int Ws, int levels) {
    CNN_REQUIRE(dataset != nullptr, "%s: null pointer", who);
    CNN_REQUIRE(N >= 1 && N <= 2147483647LL && Hs >= 1 && Hs <= kMaxDim && Ws >= 1 && Ws <= kMaxDim,
                "%s: N=%lld (1..2^31-1) images of %dx%d (each 1..8192)", who, N, Hs, Ws);
    CNN_REQUIRE(levels >= 1 && levels <= cnn_dataset_max_levels(Hs, Ws), "%s: levels=%d (1..%d for %dx%d)", who, levels,
                cnn_dataset_max_levels(Hs, Ws), Hs, Ws);
    int dev = 0;
    CNN_HIP_CHECK(hipGetDevice(&dev));
    Dataset* ds = new Dataset();
    ds->N = N; ds->Hs = Hs; ds->Ws = Ws; ds->device = dev;
    ds->sample_bytes = (size_t)Hs * Ws * 3;
    size_t bytes = 0;  // level 0 first, as ever; every offset in 64 bits
    for (int l = 0, h = Hs, w = Ws; l < levels; ++l, h = (h + 1) / 2, w = (w + 1) / 2) {
        DatasetLevel lv;
        lv.base = (long long)bytes;
        lv.H = h; lv.W = w;
        lv.sample_bytes = h * w * 3;
        lv.reserved = 0;
        ds->level.push_back(lv);
        bytes += (size_t)N * (size_t)lv.sample_bytes;
    }
    hipError_t e = hipMalloc((void**)&ds->images, bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&ds->labels, (size_t)N * sizeof(int));
    if (e == hipSuccess) e = hipMemset(ds->images, 0, bytes);  // (the all-zero image's levels are all zero)
    if (e == hipSuccess) e = hipMemset(ds->labels, 0xFF, (size_t)N * sizeof(int));  // every label -1
    if (e == hipSuccess && levels > 1) {
        e = hipMalloc((void**)&ds->table, (size_t)levels * sizeof(DatasetLevel));
        if (e == hipSuccess) e = hipMemcpy(ds->table, ds->level.data(), (size_t)levels * sizeof(DatasetLevel), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&ds->stream, hipStreamNonBlocking);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        if (ds->images) (void)hipFree(ds->images);
        if (ds->labels) (void)hipFree(ds->labels);
        if (ds->table) (void)hipFree(ds->table);
        if (ds->stream) (void)hipStreamDestroy(ds->stream);
        delete ds;
        return fail(CNN_AMD_E_HIP + (int)e, "%s: %zu bytes of images and %lld labels: %s", who, bytes, N, hipGetErrorString(e));
    }
    *dataset = ds;
    return CNN_AMD_OK;
}
}  // namespace

int cnn_dataset_create_u8(void** dataset, long long N, int Hs, int Ws) { return dataset_create("cnn_dataset_create_u8", dataset, N, Hs, Ws, 1); }

int cnn_dataset_create_u8_levels(void** dataset, long long N, int Hs, int Ws, int levels) {
    return dataset_create("cnn_dataset_create_u8_levels", dataset, N, Hs, Ws, levels);
}

namespace {
int dataset_range(const char* who, Dataset* ds, long long first, long long count, const void* images, const void* labels) {
    CNN_REQUIRE(ds != nullptr, "%s: null dataset", who);
    CNN_REQUIRE(count > 0 && first >= 0 && first < ds->N && count <= ds->N - first, "%s: samples [%lld, %lld + %lld) outside [0, %lld)", who, first, first,
                count, ds->N);
    CNN_REQUIRE(images != nullptr || labels != nullptr, "%s: images and labels are both null", who);
    return CNN_AMD_OK;
}
}  // namespace

int cnn_dataset_write(void* dataset, long long first, long long count, const unsigned char* images, const int* labels) {
    Dataset* ds = static_cast<Dataset*>(dataset);
    if (int rc = dataset_range("cnn_dataset_write", ds, first, count, images, labels)) return rc;
    std::lock_guard<std::mutex> lk(ds->mu);
    for (Stager* st : ds->stagers) CNN_HIP_CHECK(hipStreamSynchronize(st->copy));  // every submitted gather has read its bytes
    if (images) CNN_HIP_CHECK(hipMemcpy(ds->images + (size_t)first * ds->sample_bytes, images, (size_t)count * ds->sample_bytes, hipMemcpyHostToDevice));
    if (labels) CNN_HIP_CHECK(hipMemcpy(ds->labels + first, labels, (size_t)count * sizeof(int), hipMemcpyHostToDevice));
    CNN_HIP_CHECK(hipStreamSynchronize(nullptr));  // (a copy out of pageable memory may return once it is staged)
    if (images && ds->level.size() > 1) {  // the half-size levels of exactly these samples, one launch per level, behind the copy above
        for (size_t l = 1; l < ds->level.size(); ++l)
            if (int rc = dataset_halve_u8(ds->images + ds->level[l - 1].base, ds->images + ds->level[l].base, first, count, ds->level[l - 1].H,
                                          ds->level[l - 1].W, ds->stream))
                return rc;
        CNN_HIP_CHECK(hipStreamSynchronize(ds->stream));
    }
    return CNN_AMD_OK;
}

int cnn_dataset_read(void* dataset, long long first, long long count, unsigned char* images, int* labels) {
    Dataset* ds = static_cast<Dataset*>(dataset);
    if (int rc = dataset_range("cnn_dataset_read", ds, first, count, images, labels)) return rc;
    std::lock_guard<std::mutex> lk(ds->mu);
    if (images) CNN_HIP_CHECK(hipMemcpy(images, ds->images + (size_t)first * ds->sample_bytes, (size_t)count * ds->sample_bytes, hipMemcpyDeviceToHost));
    if (labels) CNN_HIP_CHECK(hipMemcpy(labels, ds->labels + first, (size_t)count * sizeof(int), hipMemcpyDeviceToHost));
    return CNN_AMD_OK;
}

int cnn_dataset_read_level(void* dataset, int level, long long first, long long count, unsigned char* images) {
    Dataset* ds = static_cast<Dataset*>(dataset);
    if (int rc = dataset_range("cnn_dataset_read_level", ds, first, count, images, nullptr)) return rc;
    CNN_REQUIRE(level >= 0 && level < (int)ds->level.size(), "cnn_dataset_read_level: level %d outside [0, %d)", level, (int)ds->level.size());
    const DatasetLevel& lv = ds->level[(size_t)level];
    std::lock_guard<std::mutex> lk(ds->mu);
    CNN_HIP_CHECK(hipMemcpy(images, ds->images + lv.base + (size_t)first * (size_t)lv.sample_bytes, (size_t)count * (size_t)lv.sample_bytes,
                            hipMemcpyDeviceToHost));
    return CNN_AMD_OK;
}

int cnn_dataset_level_info(void* dataset, int* levels, int level, int* H_l, int* W_l) {
    Dataset* ds = static_cast<Dataset*>(dataset);
    CNN_REQUIRE(ds != nullptr && (levels != nullptr || H_l != nullptr || W_l != nullptr), "cnn_dataset_level_info: null pointer");
    CNN_REQUIRE(level >= 0 && level < (int)ds->level.size(), "cnn_dataset_level_info: level %d outside [0, %d)", level, (int)ds->level.size());
    if (levels) *levels = (int)ds->level.size();
    if (H_l) *H_l = ds->level[(size_t)level].H;
    if (W_l) *W_l = ds->level[(size_t)level].W;
    return CNN_AMD_OK;
}

int cnn_dataset_info(void* dataset, long long* N, int* Hs, int* Ws) {
    Dataset* ds = static_cast<Dataset*>(dataset);
    CNN_REQUIRE(ds != nullptr && (N != nullptr || Hs != nullptr || Ws != nullptr), "cnn_dataset_info: null pointer");
    if (N) *N = ds->N;
    if (Hs) *Hs = ds->Hs;
    if (Ws) *Ws = ds->Ws;
    return CNN_AMD_OK;
}

int cnn_dataset_destroy(void* dataset) {
    Dataset* ds = static_cast<Dataset*>(dataset);
    CNN_REQUIRE(ds != nullptr, "cnn_dataset_destroy: null dataset");
    {
        std::lock_guard<std::mutex> lk(ds->mu);
        CNN_REQUIRE(ds->stagers.empty(), "cnn_dataset_destroy: %zu stager(s) still attached (cnn_batch_stager_destroy them first)", ds->stagers.size());
    }
    (void)hipFree(ds->images);
    (void)hipFree(ds->labels);
    if (ds->table) (void)hipFree(ds->table);
    if (ds->stream) (void)hipStreamDestroy(ds->stream);
    delete ds;
    return CNN_AMD_OK;
}
}  // extern "C"
