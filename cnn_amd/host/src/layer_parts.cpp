// layer_parts.cpp -- Workspace, ParamBlock and write_back_staged (include/layer_parts.h) on the C ABI's memory calls; nothing here knows a layer
#include "architectures.h"
#include "host_util.h"

using architectures::stream;

namespace cnn_amd_host {

Workspace::~Workspace() {
    if (ptr) cnn_device_free(ptr);
}

void Workspace::reserve(size_t need) {
    if (need <= bytes) return;
    if (ptr) cnn_device_free(ptr);
    ptr = nullptr;
    bytes = 0;
    ptr = dev_alloc(need);
    bytes = need;
}

void ParamBlock::release() {
    if (owned) {
        cnn_device_free(params);
        cnn_device_free(grads);
    }
    owned = false;
}

void ParamBlock::allocate(size_t count) {
    n = count;
    params = (data_type*)dev_alloc(sizeof(data_type) * n);
    grads = (data_type*)dev_alloc(sizeof(data_type) * n);
    owned = true;
}

void ParamBlock::upload(const data_type* host) {
    must(cnn_memcpy_h2d(params, host, sizeof(data_type) * n, stream), "cnn_memcpy_h2d");
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
}

void ParamBlock::adopt(data_type* params_dev, data_type* grads_dev, bool zero_grads) {
    must(cnn_memcpy_d2d(params_dev, params, sizeof(data_type) * n, stream), "cnn_memcpy_d2d");
    if (zero_grads) must(cnn_memset_zero(grads_dev, sizeof(data_type) * n, stream), "cnn_memset_zero");
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
    release();
    params = params_dev;
    grads = grads_dev;
}

void ParamBlock::save(std::ofstream& writer) const {
    std::vector<data_type> host(n);
    must(cnn_memcpy_d2h(host.data(), params, sizeof(data_type) * n, stream), "cnn_memcpy_d2h");
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
    writer.write(reinterpret_cast<const char*>(host.data()), static_cast<std::streamsize>(sizeof(data_type) * n));
}

void ParamBlock::load(std::ifstream& reader) {
    std::vector<data_type> host(n);
    reader.read(reinterpret_cast<char*>(host.data()), static_cast<std::streamsize>(sizeof(data_type) * n));
    upload(host.data());
}

void write_back_staged(std::vector<tensor>& delta, const data_type* d, size_t sample_len, int B, bool staged) {
    if (!staged) return;
    for (int b = 0; b < B; ++b) {
        const data_type* src = d + sample_len * b;
        if (delta[b]->on_device())
            must(cnn_memcpy_d2d(delta[b]->dev, src, sizeof(data_type) * sample_len, stream), "cnn_memcpy_d2d");
        else
            must(cnn_memcpy_d2h(delta[b]->data, src, sizeof(data_type) * sample_len, stream), "cnn_memcpy_d2h");
    }
    must(cnn_stream_synchronize(stream), "cnn_stream_synchronize");
}

}  // namespace cnn_amd_host
