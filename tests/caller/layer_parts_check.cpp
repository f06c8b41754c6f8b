// layer_parts_check.cpp -- the parts the host layers are made of (cnn_amd/host/include/layer_parts.h: Mark, Workspace, ParamBlock,
// write_back_staged) against stub cnn_* functions defined here: "device" memory is host memory, so AddressSanitizer sees every index.
// Built with -fsanitize=address,undefined together with layer_parts.cpp and tensor3d.cpp and run on the CPU by tests/test_layer_parts.py; it needs neither
// a device nor libcnn_amd.so.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>

#include "layer_parts.h"

namespace architectures {
void* stream = nullptr;
}

static std::set<void*> live;  // what cnn_device_alloc handed out and cnn_device_free has not seen yet
static int syncs = 0;
static int bad_frees = 0;  // double frees, pointers that were never allocated (the parts do not look at cnn_device_free's return value)
extern "C" {
const char* cnn_amd_last_error(void) { return "stub"; }
int cnn_device_alloc(void** ptr, size_t bytes) {
    *ptr = std::malloc(bytes ? bytes : 1);
    live.insert(*ptr);
    return 0;
}
int cnn_device_free(void* ptr) {
    if (live.erase(ptr) != 1) {
        ++bad_frees;
        return 1;
    }
    std::free(ptr);
    return 0;
}
int cnn_memcpy_h2d(void* dst, const void* src, size_t bytes, void*) { std::memcpy(dst, src, bytes); return 0; }
int cnn_memcpy_d2h(void* dst, const void* src, size_t bytes, void*) { std::memcpy(dst, src, bytes); return 0; }
int cnn_memcpy_d2d(void* dst, const void* src, size_t bytes, void*) { std::memcpy(dst, src, bytes); return 0; }
int cnn_memset_zero(void* dst, size_t bytes, void*) { std::memset(dst, 0, bytes); return 0; }
int cnn_stream_synchronize(void*) { ++syncs; return 0; }
}

#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

using namespace cnn_amd_host;

int main(int argc, char** argv) {
    {  // Mark: one-shot
        Mark m;
        CHECK(!m.armed() && !m.take());
        m.arm();
        CHECK(m.armed() && m.take() && !m.armed() && !m.take());
        m.set(true);
        m.clear();
        CHECK(!m.take());
    }
    {  // Workspace: grows, never shrinks, frees what it replaces and what it holds at the end
        Workspace ws;
        ws.reserve(0);
        CHECK(ws.ptr == nullptr && live.empty());
        ws.reserve(64);
        void* first = ws.ptr;
        std::memset(ws.ptr, 1, 64);
        ws.reserve(16);
        CHECK(ws.ptr == first && ws.bytes == 64);
        ws.reserve(4096);
        CHECK(ws.bytes == 4096 && live.size() == 1);
        std::memset(ws.ptr, 2, 4096);
    }
    CHECK(live.empty() && bad_frees == 0);
    {  // ParamBlock: own blocks -> the caller's blocks; a checkpoint round trip
        const size_t n = 37;
        std::vector<data_type> host(n), arena_p(n, -1.f), arena_g(n, 5.f);
        for (size_t i = 0; i < n; ++i) host[i] = (data_type)i;
        ParamBlock pb;
        pb.allocate(n);
        pb.upload(host.data());
        CHECK(live.size() == 2 && pb.of_last_forward() == pb.params);
        pb.adopt(arena_p.data(), arena_g.data(), /*zero_grads=*/true);
        CHECK(live.empty() && !pb.owned && arena_p == host && arena_g == std::vector<data_type>(n, 0.f));
        const bool stepped = true;
        pb.snapshot = host.data();
        pb.snapshot_active = &stepped;
        CHECK(pb.of_last_forward() == host.data());
        const char* path = argc > 1 ? argv[1] : "layer_parts_check.bin";
        {
            std::ofstream w(path, std::ios::binary);
            pb.save(w);
        }
        arena_p.assign(n, 0.f);
        std::ifstream r(path, std::ios::binary);
        pb.load(r);
        CHECK(arena_p == host);
        std::remove(path);
    }  // (~ParamBlock must not free the caller's blocks)
    CHECK(live.empty() && bad_frees == 0);
    {  // write_back_staged: host tensors and device views, odd sample length, more than one sample
        const size_t len = 3 * 5 * 7;
        const int B = 3;
        std::vector<data_type> staged(len * B), dev1(len, 0.f);
        for (size_t i = 0; i < staged.size(); ++i) staged[i] = (data_type)i;
        std::vector<tensor> delta;
        delta.emplace_back(new Tensor3D(3, 5, 7, "host_0"));
        delta.push_back(Tensor3D::device_view(3, 5, 7, dev1.data(), "view_1"));
        delta.emplace_back(new Tensor3D(3, 5, 7, "host_2"));
        const int before = syncs;
        write_back_staged(delta, staged.data(), len, B, /*staged=*/false);
        CHECK(syncs == before && dev1[0] == 0.f);
        write_back_staged(delta, staged.data(), len, B, /*staged=*/true);
        CHECK(syncs == before + 1);
        for (int b = 0; b < B; ++b)
            for (size_t i = 0; i < len; ++i) CHECK((b == 1 ? dev1[i] : delta[b]->data[i]) == staged[len * b + i]);
    }
    CHECK(bad_frees == 0 && live.empty());
    std::puts("ok");
    return 0;
}
