// depthwise_caller.cpp -- what a reference user writes to build and train a depthwise-separable block with the public Layer API
// (architectures::DepthwiseConv2D beside Conv2D / BatchNorm2D / ReLU in a Sequential), the MobileNet-V1-shaped
// builder, and the bare C ABI underneath (CNN_CONV2D_DEPTHWISE in cnn_conv2d_desc.flags).  tests/test_depthwise_compile.py compiles
// it against the public headers; nothing here is run.
#include <cstddef>
#include <fstream>
#include <string>
#include <vector>

#include "architectures.h"

// a MobileNet-style block list: 3x3 stem, then depthwise 3x3 + pointwise 1x1 twice, the second one down-sampling
void build_separable(architectures::Sequential& net, const int classes) {
    using namespace architectures;
    net.add(new Conv2D("conv_layer_1", 3, 8, 3, 2, 1));
    net.add(new BatchNorm2D("bn_layer_1", 8));
    net.add(new ReLU("relu_layer_1"));
    net.add(new DepthwiseConv2D("dw_layer_2", 8));  // 3x3, stride 1, pad 1
    net.add(new BatchNorm2D("bn_layer_2", 8));
    net.add(new ReLU("relu_layer_2"));
    net.add(new Conv2D("conv_layer_3", 8, 16, 1, 1, 0));
    net.add(new ReLU("relu_layer_3"));
    net.add(new DepthwiseConv2D("dw_layer_4", 16, 3, 2, 1));
    net.add(new ReLU("relu_layer_4"));
    net.add(new MaxPool2D("max_pool_1", 2, 2));
    net.add(new LinearLayer("linear_1", 16 * 4 * 4, classes));
    net.finalize();
}

int train(architectures::Sequential& net, const std::vector<tensor>& batch, const int* labels_dev, const data_type learning_rate) {
    net.set_adam(0.9f, 0.999f, 1e-8f, 1e-2f, /*decoupled=*/true);  // the dw weights decay, their biases do not
    net.train_step(batch, labels_dev, learning_rate);
    return net.num_params() > 0 ? 0 : -1;
}

// the layer alone, the way the reference drives its layers
std::vector<tensor> layer_alone(const std::vector<tensor>& input, std::vector<tensor>& delta, std::ofstream& writer) {
    architectures::DepthwiseConv2D dw("dw", 32, 5, 2, 2);
    architectures::Layer& layer = dw;
    const std::vector<tensor> out = layer.forward(input);
    std::vector<tensor> dx = layer.backward(delta);
    layer.update_gradients(1e-3f);
    layer.save_weights(writer);
    architectures::Layer::RangeList decayed, tensors;
    layer.decay_ranges(/*bias_and_norm=*/false, decayed);
    layer.param_tensors(tensors);
    const bool ok = layer.param_count() == 32 * 25 + 32 && decayed.size() == 1 && tensors.size() == 2 && !layer.get_output().empty();
    return ok ? dx : out;
}

void whole_stack(architectures::Sequential& net) { architectures::build_mobilenet_v1(net, 3, true); }

// the C ABI: one desc, the plain entry points
int by_hand(const float* x, const float* w, const float* bias, const float* dy, float* y, float* gw, float* gb, float* dx, void* ws, size_t ws_bytes) {
    const cnn_conv2d_desc d{64, 512, 14, 14, 512, 3, 1, 1, CNN_CONV2D_DEPTHWISE};
    if (cnn_conv2d_backward_workspace_bytes(&d) > ws_bytes) return -1;
    if (const int rc = cnn_conv2d_forward(&d, x, w, bias, y, ws, ws_bytes, architectures::stream)) return rc;
    return cnn_conv2d_backward(&d, x, dy, w, gw, gb, dx, 64.f, ws, ws_bytes, architectures::stream, /*defer_join=*/0);
}
