// layer_parts.h -- the parts the layer classes of architectures.h are made of (held by value; defined in src/layer_parts.cpp)
#ifndef CNN_AMD_LAYER_PARTS_H
#define CNN_AMD_LAYER_PARTS_H

#include <fstream>
#include <vector>

#include "data_format.h"

namespace cnn_amd_host {

// A fusion hand-over between neighbouring layers: a per-layer ONE-SHOT mark that says "this pass' forward (or backward) of the owner was
// already done by a neighbour's kernel".  One lifecycle for every mark:
//   1. only the owner's forward() -- for a forward mark -- or backward() -- for a backward mark -- consumes it, through take();
//   2. the owner's forward() clears (or states anew) all of the owner's backward marks, also when that forward is itself a fused
//      pass-through: no backward mark outlives the pass it was armed in;
//   3. a layer that can arm a neighbour's mark states its value on EVERY call of that kind: cleared on entry, armed on the fused branch.
// Neighbours and the container may look at a mark (armed()), never take it.
struct Mark {
    bool on = false;
    void arm() { on = true; }
    void clear() { on = false; }
    void set(bool v) { on = v; }
    bool armed() const { return on; }
    bool take() {
        const bool was = on;
        on = false;
        return was;
    }
};

// A device scratch buffer that only ever grows.
struct Workspace {
    void* ptr = nullptr;
    size_t bytes = 0;
    Workspace() = default;
    Workspace(const Workspace&) = delete;
    Workspace& operator=(const Workspace&) = delete;
    ~Workspace();
    void reserve(size_t need);
};

// A layer's parameter block and its gradient block (n floats each, checkpoint order): the layer's own until a container moves them into
// its arena (adopt).  `snapshot` is the container's copy of the block from before its latest SGD step, `*snapshot_active` whether that
// step came after the last forward pass; `lost`: the parameters the last forward pass used are gone (written from outside, or stepped
// twice without a forward pass in between) -- an output that pass did not write can no longer be re-computed.
struct ParamBlock {
    data_type* params = nullptr;
    data_type* grads = nullptr;
    size_t n = 0;
    bool owned = false;
    const data_type* snapshot = nullptr;
    const bool* snapshot_active = nullptr;
    bool lost = false;
    ParamBlock() = default;
    ParamBlock(const ParamBlock&) = delete;
    ParamBlock& operator=(const ParamBlock&) = delete;
    ~ParamBlock() { release(); }
    void release();                     // frees the blocks when they are the layer's own
    void allocate(size_t count);        // two device blocks of `count` floats, owned
    void upload(const data_type* host);  // n floats into params; synchronises
    // moves the parameters into the caller's blocks and works there from now on
    void adopt(data_type* params_dev, data_type* grads_dev, bool zero_grads);
    void save(std::ofstream& writer) const;
    void load(std::ifstream& reader);
    // the parameters the last forward pass used: the container's snapshot when its SGD step has run since
    const data_type* of_last_forward() const { return (snapshot != nullptr && snapshot_active != nullptr && *snapshot_active) ? snapshot : params; }
};

// an in-place backward pass that ran on a STAGED copy `d` of the caller's delta (host tensors, or scattered views): write the result back
void write_back_staged(std::vector<tensor>& delta, const data_type* d, size_t sample_len, int B, bool staged);

}  // namespace cnn_amd_host

#endif  // CNN_AMD_LAYER_PARTS_H
