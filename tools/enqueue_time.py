"""How long does the host take to ENQUEUE one train step (ctypes + HIP launches) vs the GPU time of the step?
--conv B,Ci,H,W,Co,k,s,pad: the host time of one cnn_conv2d_forward call on that desc instead (two launches on the implicit GEMM: the
filter re-arrangement and the tile), as the median / min / max over 20 windows of 200 calls; CNN_AMD_LIB selects the build."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

if "--conv" in sys.argv:
    from cnn_amd import capi

    case = tuple(int(v) for v in sys.argv[sys.argv.index("--conv") + 1].split(","))
    conv = capi.Conv2d(*case)
    x = torch.rand((case[0], case[1], case[2], case[3]), device="cuda")
    w = torch.rand((case[4], case[1], case[5], case[5]), device="cuda")
    b = torch.rand((case[4],), device="cuda")
    y = torch.empty(conv.out_shape(), device="cuda")
    capi.kernel_timing(1)
    conv.forward(x, w, b, y)
    torch.cuda.synchronize()
    names = list(capi.kernel_timing_report())
    capi.kernel_timing(0)
    for _ in range(200):
        conv.forward(x, w, b, y)
    torch.cuda.synchronize()
    us = []
    for _ in range(20):
        t0 = time.perf_counter()
        for _ in range(200):
            conv.forward(x, w, b, y)
        us.append(1e6 * (time.perf_counter() - t0) / 200)
        torch.cuda.synchronize()
    us.sort()
    print(f"enqueue {us[len(us) // 2]:.2f} us/call (min {us[0]:.2f}, max {us[-1]:.2f})   {names}")
    sys.exit(0)

from cnn_amd.pynet import AlexNetHip

B = 256
net = AlexNetHip(B, 3)
net.load_params((torch.randn(net.n_params) * 0.1).numpy())
x = torch.rand((B, 3, 224, 224), device="cuda")
labels = torch.randint(0, 3, (B,), dtype=torch.int32, device="cuda")
for _ in range(5):
    net.train_step(x, labels, 1e-3)
torch.cuda.synchronize()
n = 50
t0 = time.perf_counter()
for _ in range(n):
    net.train_step(x, labels, 1e-3)
t1 = time.perf_counter()
torch.cuda.synchronize()
t2 = time.perf_counter()
print(f"enqueue {1e3*(t1-t0)/n:.3f} ms/step   total {1e3*(t2-t0)/n:.3f} ms/step")
