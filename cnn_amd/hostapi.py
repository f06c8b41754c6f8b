"""ctypes front end of libcnn_amd_host.so -- the C++17 mirror of the reference's Layer/AlexNet API
(cnn_amd/host).  Used by tests/ and bench.py to drive exactly the code path a reference user links against."""
import contextlib
import ctypes as C
import os

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcnn_amd_host.so")
_lib = None

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int)
SIGNATURES = {
    "cnnh_net_create": (C.c_void_p, [C.c_int, C.c_void_p, C.c_void_p]),
    "cnnh_net_create_ex": (C.c_void_p, [C.c_int, C.c_void_p, C.c_void_p, C.c_int]),
    "cnnh_seq_create": (C.c_void_p, [C.c_int, C.c_int]),
    "cnnh_seq_add_conv": (None, [C.c_void_p, C.c_char_p] + [C.c_int] * 5),
    "cnnh_seq_add_dwconv": (None, [C.c_void_p, C.c_char_p] + [C.c_int] * 4),
    "cnnh_seq_add_bn": (None, [C.c_void_p, C.c_char_p, C.c_int]),
    "cnnh_seq_add_relu": (None, [C.c_void_p, C.c_char_p]),
    "cnnh_seq_add_dropout": (None, [C.c_void_p, C.c_char_p, C.c_float]),
    "cnnh_seq_add_pool": (None, [C.c_void_p, C.c_char_p, C.c_int, C.c_int]),
    "cnnh_seq_add_linear": (None, [C.c_void_p, C.c_char_p, C.c_int, C.c_int]),
    "cnnh_seq_finalize": (None, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cnnh_stack_create": (C.c_void_p, [C.c_char_p, C.c_int, C.c_int]),
    "cnnh_net_describe": (C.c_size_t, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "cnnh_net_set_comm": (None, [C.c_void_p, C.c_void_p, C.c_int]),
    "cnnh_net_allreduce_gradients": (None, [C.c_void_p]),
    "cnnh_net_update_auto": (None, [C.c_void_p, C.c_float]),
    "cnnh_net_destroy": (None, [C.c_void_p]),
    "cnnh_net_num_params": (C.c_size_t, [C.c_void_p]),
    "cnnh_net_params_device": (C.c_void_p, [C.c_void_p]),
    "cnnh_net_grads_device": (C.c_void_p, [C.c_void_p]),
    "cnnh_net_set_optimizer": (None, [C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int]),
    "cnnh_net_velocity_device": (C.c_void_p, [C.c_void_p]),
    "cnnh_net_get_velocity": (C.c_int, [C.c_void_p, _F]),
    "cnnh_net_set_adam": (None, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]),
    "cnnh_net_adam_m_device": (C.c_void_p, [C.c_void_p]),
    "cnnh_net_adam_v_device": (C.c_void_p, [C.c_void_p]),
    "cnnh_net_get_adam_state": (C.c_int, [C.c_void_p, _F, _F, C.POINTER(C.c_uint64)]),
    "cnnh_net_set_grad_clip": (None, [C.c_void_p, C.c_float]),
    "cnnh_net_set_lamb": (None, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int]),
    "cnnh_net_set_lars": (None, [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]),
    "cnnh_net_segment_count": (C.c_size_t, [C.c_void_p]),
    "cnnh_net_layerwise_active": (C.c_int, [C.c_void_p]),
    "cnnh_net_get_segments": (None, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cnnh_net_get_trust_stats": (C.c_int, [C.c_void_p, _F, _F, _F]),
    "cnnh_net_last_grad_norm": (C.c_int, [C.c_void_p, _F, _F]),
    "cnnh_net_set_grad_accumulation": (None, [C.c_void_p, C.c_int]),
    "cnnh_net_accumulation_phase": (C.c_int, [C.c_void_p]),
    "cnnh_net_get_accumulated_grads": (C.c_int, [C.c_void_p, _F]),
    "cnnh_net_set_ema": (None, [C.c_void_p, C.c_float, C.c_int, C.c_int]),
    "cnnh_net_reset_ema": (None, [C.c_void_p]),
    "cnnh_net_get_ema": (C.c_int, [C.c_void_p, _F]),
    "cnnh_net_ema_updates": (C.c_uint64, [C.c_void_p]),
    "cnnh_net_swap_ema": (None, [C.c_void_p]),
    "cnnh_net_ema_swapped": (C.c_int, [C.c_void_p]),
    "cnnh_net_save_ema_state": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cnnh_net_load_ema_state": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cnnh_net_save_optimizer_state": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cnnh_net_load_optimizer_state": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cnnh_set_stream": (None, [C.c_void_p]),
    "cnnh_set_no_grad": (None, [C.c_int]),
    "cnnh_set_fuse_layers": (None, [C.c_int]),
    "cnnh_set_fuse_pool_block": (None, [C.c_int]),
    "cnnh_set_input_gradient": (None, [C.c_int]),
    "cnnh_net_set_params": (None, [C.c_void_p, _F]),
    "cnnh_net_get_params": (None, [C.c_void_p, _F]),
    "cnnh_net_get_grads": (None, [C.c_void_p, _F]),
    "cnnh_net_load_checkpoint": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cnnh_net_save_checkpoint": (None, [C.c_void_p, C.c_char_p]),
    "cnnh_net_forward_host": (None, [C.c_void_p, _F, C.c_int, C.c_int, C.c_int, _F]),
    "cnnh_net_train_step_host": (C.c_float, [C.c_void_p, _F, _I, C.c_int, C.c_int, C.c_int, C.c_float, _F]),
    "cnnh_net_train_step_device": (C.c_float, [C.c_void_p, C.c_void_p, _I, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int]),
    "cnnh_net_update": (None, [C.c_void_p, C.c_float, C.c_float]),
    "cnnh_net_train_step_device_loss": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float]),
    "cnnh_net_forward_backward_device_loss": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "cnnh_net_last_loss": (C.c_float, [C.c_void_p]),
    "cnnh_net_set_label_smoothing": (None, [C.c_void_p, C.c_float]),
    "cnnh_net_train_step_mixed": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(capi.MixDesc), C.c_float]),
    "cnnh_net_train_step_soft": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float]),
    "cnnh_net_get_targets": (C.c_int, [C.c_void_p, _F, C.c_int]),
    "cnnh_net_eval_begin": (None, [C.c_void_p, C.c_int]),
    "cnnh_net_eval_step_device": (None, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "cnnh_net_eval_result": (None, [C.c_void_p, C.POINTER(capi.EvalResult), C.c_void_p]),
    "cnnh_net_get_predictions": (C.c_int, [C.c_void_p, _I, C.c_int]),
    "cnnh_net_flush": (None, [C.c_void_p]),
    "cnnh_net_input_delta": (C.c_int, [C.c_void_p, _F, C.c_size_t]),
    "cnnh_net_layer_output": (C.c_int, [C.c_void_p, C.c_char_p, _F, C.c_size_t]),
    "cnnh_net_grad_cam": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t, _F, C.c_size_t]),
}


def load():
    global _lib
    if _lib is None:
        capi.load()  # libcnn_amd.so first (the host library links against it)
        if os.environ.get("CNN_AMD_LIB"):
            raise capi.CnnAmdError("CNN_AMD_LIB selects another build of the C ABI; libcnn_amd_host.so is linked against the in-tree libcnn_amd.so")
        if not os.path.exists(LIB_PATH):
            raise capi.CnnAmdError(f"{LIB_PATH} is missing: run __graft_entry__.build()")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _fp(a):
    return a.ctypes.data_as(_F)


def mix_params(rng, H, W, mixup_alpha=0.8, cutmix_alpha=1.0, switch_prob=0.5, pair_rule=capi.PAIR_FLIP, pair_shift=0):
    """One batch's mixing parameters, sampled on the host the way timm's Mixup does: lam ~ Beta(a, a) from `rng` (a
    numpy.random.Generator); CutMix with probability switch_prob when both alphas are positive (always when only cutmix_alpha is),
    mixup otherwise.  CutMix: a box of side ratio sqrt(1 - lam) around a uniform centre, clipped to the plane; the descriptor's lam is
    then the clipped box's own (cnn_cutmix_lambda).  Returns a capi.MixDesc for HostNet.train_step_mixed / capi.batch_mix."""
    if mixup_alpha <= 0 and cutmix_alpha <= 0:
        raise capi.CnnAmdError("mix_params: one of mixup_alpha and cutmix_alpha must be positive")
    use_cutmix = cutmix_alpha > 0 and (mixup_alpha <= 0 or float(rng.random()) < switch_prob)
    alpha = cutmix_alpha if use_cutmix else mixup_alpha
    lam = min(1.0, max(0.0, float(rng.beta(alpha, alpha))))
    if not use_cutmix:
        return capi.MixDesc(capi.MIX_MIXUP, lam, pair_rule, pair_shift, 0, 0, 0, 0)
    ratio = float(np.sqrt(1.0 - lam))
    cut_h, cut_w = int(H * ratio), int(W * ratio)
    cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
    y0, y1 = min(max(cy - cut_h // 2, 0), H), min(max(cy + cut_h // 2, 0), H)
    x0, x1 = min(max(cx - cut_w // 2, 0), W), min(max(cx + cut_w // 2, 0), W)
    return capi.MixDesc(capi.MIX_CUTMIX, capi.cutmix_lambda(H, W, y0, y1, x0, x1), pair_rule, pair_shift, y0, y1, x0, x1)


def augment_params(rng, B, Hs, Ws, H, W, hflip=0.5, vflip=0.2, crop=0.7, rotate=0.6, crop_min=0.7, max_angle=15.0):
    """One batch's augmentation maps, sampled on the host the way the reference's ImageAugmentor::make_augment does (pipeline.cpp:40-77)
    with `rng` (a numpy.random.Generator): per sample the four ops in a shuffled order, each firing with its own probability; crop: a
    ratio uniform in [crop_min, 1] of the current canvas at a uniform position, rotate: an angle uniform in [-max_angle, max_angle]
    degrees.  Composition goes through capi.augment_matrix (ops in order, then the resize to H x W).  Returns a (B, 6) float32 array
    for BatchStager.matrices(slot) / capi.augment_u8."""
    probs = {capi.AUG_HFLIP: hflip, capi.AUG_VFLIP: vflip, capi.AUG_CROP: crop, capi.AUG_ROTATE: rotate}
    kinds = np.array(sorted(probs))
    out = np.empty((B, 6), dtype=np.float32)
    for b in range(B):
        ops, cw, ch = [], int(Ws), int(Hs)
        for kind in rng.permutation(kinds):
            if not float(rng.random()) < probs[int(kind)]:
                continue
            if kind == capi.AUG_CROP:
                ratio = float(rng.uniform(crop_min, 1.0))
                w, h = max(1, int(cw * ratio)), max(1, int(ch * ratio))
                x0, y0 = int(rng.integers(0, cw - w + 1)), int(rng.integers(0, ch - h + 1))
                ops.append((capi.AUG_CROP, x0, y0, w, h))
                cw, ch = w, h
            elif kind == capi.AUG_ROTATE:
                ops.append((capi.AUG_ROTATE, float(rng.uniform(-max_angle, max_angle))))
            else:
                ops.append((int(kind),))
        out[b] = capi.augment_matrix(ops, Hs, Ws, H, W)
    return out


def photo_params(rng, B, H, W, brightness=0.4, contrast=0.4, saturation=0.4, hue=0.0, pivot=0.5, erase_prob=0.25, erase_area=(0.02, 1 / 3),
                 erase_aspect=(0.3, 3.3), erase_value="const"):
    """One batch's photometric parameters for an H x W output, sampled on the host with `rng` (a numpy.random.Generator).  Returns a
    (B, 20) float32 array for BatchStager.photo(slot): A[9], o[3], ex0, ey0, ew, eh, ev[3], 0.

    Colour follows torchvision's ColorJitter sampling: per sample the four ops in a shuffled order; brightness, contrast and saturation
    factors uniform in [max(0, 1 - a), 1 + a]; hue uniform in [-hue, hue] as a fraction of the colour wheel (at most 0.5; 360 degrees
    times it).  An amplitude of 0 leaves its op out.  Composition goes through capi.colour_matrix: contrast pivots on the fixed `pivot`
    (not the image's mean grey), hue is the linear YIQ rotation (not the HSV shift), and nothing clamps between the ops.

    Erasing follows timm's RandomErasing sampling: with probability erase_prob, up to 10 attempts of an area fraction uniform in
    erase_area and an aspect ratio log-uniform in erase_aspect, h = round(sqrt(area * aspect)), w = round(sqrt(area / aspect)); the
    first box with 1 <= w < W and 1 <= h < H is placed at a uniform position where it fits; no fitting attempt, no box.  The box's
    value is in OUTPUT units (behind the normalisation): "const" is 0, "rand" draws one standard normal value per channel here on the
    host.  Per-pixel noise (timm's mode="pixel") is out of scope: the kernel writes one value per channel and box."""
    if erase_value not in ("const", "rand"):
        raise capi.CnnAmdError('photo_params: erase_value is "const" or "rand"')
    if not 0.0 <= hue <= 0.5:
        raise capi.CnnAmdError("photo_params: hue is a fraction of the colour wheel, 0 .. 0.5")
    amps = {capi.COL_BRIGHTNESS: brightness, capi.COL_CONTRAST: contrast, capi.COL_SATURATION: saturation, capi.COL_HUE: hue}
    kinds = np.array(sorted(amps))
    out = np.zeros((B, capi.PHOTO_FLOATS), dtype=np.float32)
    log_aspect = (np.log(erase_aspect[0]), np.log(erase_aspect[1]))
    for b in range(B):
        ops = []
        for kind in rng.permutation(kinds):
            a = float(amps[int(kind)])
            if a == 0.0:
                continue
            if kind == capi.COL_HUE:
                ops.append((capi.COL_HUE, 360.0 * float(rng.uniform(-a, a))))
            elif kind == capi.COL_CONTRAST:
                ops.append((capi.COL_CONTRAST, float(rng.uniform(max(0.0, 1.0 - a), 1.0 + a)), float(pivot)))
            else:
                ops.append((int(kind), float(rng.uniform(max(0.0, 1.0 - a), 1.0 + a))))
        out[b, :12] = capi.colour_matrix(ops)
        if not float(rng.random()) < erase_prob:
            continue
        for _ in range(10):
            target = float(rng.uniform(erase_area[0], erase_area[1])) * H * W
            aspect = float(np.exp(rng.uniform(log_aspect[0], log_aspect[1])))
            h, w = int(round(np.sqrt(target * aspect))), int(round(np.sqrt(target / aspect)))
            if 1 <= w < W and 1 <= h < H:
                out[b, 12:16] = (int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h)
                if erase_value == "rand":
                    out[b, 16:19] = rng.standard_normal(3)
                break
    return out


def epoch_order(n, batch, seed, epoch, shuffle=True, drop_last=False, rank=0, world=1):
    """The sample indices of one epoch over a resident dataset of n samples, for rank `rank` of `world`: an int32 [steps][batch] array
    for BatchStager.indices(slot), row by row.  The permutation of range(n) is drawn from (seed, epoch) alone -- the same on every rank,
    another one every epoch; shuffle=False is the ascending order.  Rank r takes elements r, r + world, ... of it.  Every rank gets the
    same number of rows: without drop_last the tail is padded with -1 ("no sample": a fill image with label -1, which evaluation counts
    as ignored and training must not see); with drop_last only the rows that every rank can fill are kept.  Pure NumPy, no device."""
    n, batch, rank, world = int(n), int(batch), int(rank), int(world)
    if n < 1 or batch < 1 or world < 1 or not 0 <= rank < world:
        raise capi.CnnAmdError(f"epoch_order: n={n}, batch={batch} (each >= 1), rank={rank} of world={world}")
    perm = np.random.default_rng([int(seed), int(epoch)]).permutation(n) if shuffle else np.arange(n)
    mine = perm[rank::world].astype(np.int32)
    if drop_last:
        steps = (n // world) // batch  # (the smallest share)
        return np.ascontiguousarray(mine[:steps * batch].reshape(steps, batch))
    largest = (n + world - 1) // world  # (the largest share)
    steps = (largest + batch - 1) // batch
    out = np.full(steps * batch, -1, dtype=np.int32)
    out[:mine.size] = mine
    return out.reshape(steps, batch)


class HostNet:
    """architectures::Sequential / AlexNet (cnn_amd/host) behind a handle: the C++ Layer API a reference user links against."""

    h = None

    def _adopt(self, handle, classes, params, grads):
        self.classes = classes
        self._keep = (params, grads)  # torch tensors that own the arenas, if any
        self.h = C.c_void_p(handle)
        self.n_params = int(self.lib.cnnh_net_num_params(self.h))

    def describe(self):
        """[(layer name, parameter count)] in layer order"""
        n = int(self.lib.cnnh_net_describe(self.h, None, 0))
        buf = C.create_string_buffer(n)
        self.lib.cnnh_net_describe(self.h, buf, n)
        return [(ln.rsplit(":", 1)[0], int(ln.rsplit(":", 1)[1])) for ln in buf.value.decode().splitlines()]

    def set_comm(self, comm, world):
        """comm: the void* of cnn_comm_init_rank / cnn_comm_init_all (int or ctypes.c_void_p), or None"""
        self.lib.cnnh_net_set_comm(self.h, comm, int(world))

    def allreduce_gradients(self):
        self.lib.cnnh_net_allreduce_gradients(self.h)

    def update_auto(self, lr):
        """Sequential::update_gradients(lr): all-reduce + lr/world when a communicator is set"""
        self.lib.cnnh_net_update_auto(self.h, float(lr))

    def close(self):
        if self.h:
            self.lib.cnnh_net_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        assert flat.size == self.n_params
        self.lib.cnnh_net_set_params(self.h, _fp(flat))

    def get_params(self):
        out = np.empty(self.n_params, np.float32)
        self.lib.cnnh_net_get_params(self.h, _fp(out))
        return out

    def get_grads(self):
        out = np.empty(self.n_params, np.float32)
        self.lib.cnnh_net_get_grads(self.h, _fp(out))
        return out

    def load_checkpoint(self, path):
        if self.lib.cnnh_net_load_checkpoint(self.h, str(path).encode()) != 0:
            raise FileNotFoundError(path)

    def save_checkpoint(self, path):
        self.lib.cnnh_net_save_checkpoint(self.h, str(path).encode())

    def set_optimizer(self, momentum, weight_decay=0.0, nesterov=False, decay_bias_and_norm=False):
        """Sequential::set_optimizer: SGD with momentum / weight decay / Nesterov for every later step on the arena;
        set_optimizer(0, 0) returns to the plain step"""
        self.lib.cnnh_net_set_optimizer(self.h, float(momentum), float(weight_decay), 1 if nesterov else 0, 1 if decay_bias_and_norm else 0)

    def velocity_ptr(self):
        """device pointer of the velocity arena (n_params floats); None before the first set_optimizer"""
        return self.lib.cnnh_net_velocity_device(self.h)

    def get_velocity(self):
        out = np.empty(self.n_params, np.float32)
        if self.lib.cnnh_net_get_velocity(self.h, _fp(out)) != 0:
            raise capi.CnnAmdError("get_velocity before set_optimizer")
        return out

    def set_adam(self, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False, decay_bias_and_norm=False):
        """Sequential::set_adam: Adam (decoupled=False: L2 term in the gradient) or AdamW (decoupled=True) for every later step on the
        arena; replaces set_optimizer and is replaced by it, the moments and the step counter survive a switch"""
        self.lib.cnnh_net_set_adam(self.h, float(beta1), float(beta2), float(eps), float(weight_decay), 1 if decoupled else 0,
                                   1 if decay_bias_and_norm else 0)

    def adam_ptrs(self):
        """device pointers of exp_avg and exp_avg_sq (n_params floats each); (None, None) before the first set_adam"""
        return self.lib.cnnh_net_adam_m_device(self.h), self.lib.cnnh_net_adam_v_device(self.h)

    def get_adam_state(self):
        """(exp_avg, exp_avg_sq, step): the moments on the host and the number of container steps taken under Adam"""
        m, v = np.empty(self.n_params, np.float32), np.empty(self.n_params, np.float32)
        step = C.c_uint64(0)
        if self.lib.cnnh_net_get_adam_state(self.h, _fp(m), _fp(v), C.byref(step)) != 0:
            raise capi.CnnAmdError("get_adam_state before set_adam")
        return m, v, int(step.value)

    def set_grad_clip(self, max_norm):
        """Sequential::set_grad_clip: clip every later step's gradient arena to this global L2 norm (0: off); a clipped train step
        takes the plain sequence instead of the fused tail"""
        self.lib.cnnh_net_set_grad_clip(self.h, float(max_norm))

    def last_grad_norm(self):
        """(total norm, coefficient) of the latest clipped step; synchronises"""
        norm, coef = np.zeros(1, np.float32), np.zeros(1, np.float32)
        if self.lib.cnnh_net_last_grad_norm(self.h, _fp(norm), _fp(coef)) != 0:
            raise capi.CnnAmdError("last_grad_norm before set_grad_clip")
        return norm[0], coef[0]

    def set_lamb(self, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.0, decay_bias_and_norm=False, adapt_bias_and_norm=False):
        """Sequential::set_lamb: LAMB (Adam's moments, a trust ratio per parameter tensor) for every later step on the arena; shares
        the moments and the step counter with set_adam.  A layer-wise step is one call over the whole arena: no fused step tail."""
        self.lib.cnnh_net_set_lamb(self.h, float(beta1), float(beta2), float(eps), float(weight_decay), 1 if decay_bias_and_norm else 0,
                                   1 if adapt_bias_and_norm else 0)

    def set_lars(self, momentum, weight_decay=0.0, trust_coefficient=1e-3, eps=1e-8, nesterov=False, decay_bias_and_norm=False,
                 adapt_bias_and_norm=False):
        """Sequential::set_lars: LARS (momentum SGD, a trust ratio per parameter tensor) for every later step on the arena; shares the
        velocity with set_optimizer"""
        self.lib.cnnh_net_set_lars(self.h, float(momentum), float(weight_decay), float(trust_coefficient), float(eps), 1 if nesterov else 0,
                                   1 if decay_bias_and_norm else 0, 1 if adapt_bias_and_norm else 0)

    def layerwise_active(self):
        return self.lib.cnnh_net_layerwise_active(self.h) != 0

    def segment_count(self):
        """number of parameter tensors in the segment table; 0 before the first set_lamb / set_lars"""
        return int(self.lib.cnnh_net_segment_count(self.h))

    def segment_table(self):
        """(bounds, flags): segment_count + 1 ascending arena offsets from 0 to n_params, capi.SEG_DECAY | capi.SEG_ADAPT per tensor"""
        ns = self.segment_count()
        bounds, flags = np.zeros(ns + 1, np.uint32), np.zeros(ns, np.uint32)
        if ns:
            self.lib.cnnh_net_get_segments(self.h, bounds.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p))
        return bounds, flags

    def trust_stats(self):
        """(w_norm, u_norm, ratio) per parameter tensor of the latest layer-wise step; synchronises"""
        ns = self.segment_count()
        w, u, r = (np.zeros(max(ns, 1), np.float32) for _ in range(3))
        if self.lib.cnnh_net_get_trust_stats(self.h, _fp(w), _fp(u), _fp(r)) != 0:
            raise capi.CnnAmdError("trust_stats before set_lamb / set_lars")
        return w[:ns], u[:ns], r[:ns]

    def set_grad_accumulation(self, micro_steps):
        """Sequential::set_grad_accumulation: every later container step counts one micro-batch, the optimizer steps once per
        micro_steps of them on their summed gradients (1: off); an open window is discarded.  No fused step tail while it is on."""
        if int(micro_steps) < 1:
            raise capi.CnnAmdError(f"set_grad_accumulation({micro_steps}): at least 1")
        self.lib.cnnh_net_set_grad_accumulation(self.h, int(micro_steps))

    def accumulation_phase(self):
        """micro-batches in the open window, 0 .. micro_steps - 1"""
        return int(self.lib.cnnh_net_accumulation_phase(self.h))

    def get_accumulated_grads(self):
        """the accumulator on the host: the sum over the open window's micro-batches -- after a closing call the closed window's sum,
        clipped when clipping is on"""
        out = np.empty(self.n_params, np.float32)
        if self.lib.cnnh_net_get_accumulated_grads(self.h, _fp(out)) != 0:
            raise capi.CnnAmdError("get_accumulated_grads before set_grad_accumulation(k > 1)")
        return out

    def set_ema(self, decay, warmup=False, average_stats=False):
        """Sequential::set_ema: a shadow copy of the arena follows every later optimizer step, shadow = d * shadow + (1 - d) * params
        (0: off, the shadow stays); warmup: d = min(decay, (1 + t) / (10 + t)); BatchNorm2D's moving statistics are copied, not
        averaged, unless average_stats.  No fused step tail while it is on."""
        if not 0.0 <= float(decay) < 1.0:
            raise capi.CnnAmdError(f"set_ema({decay}): decay in [0, 1)")
        self.lib.cnnh_net_set_ema(self.h, float(decay), 1 if warmup else 0, 1 if average_stats else 0)

    def reset_ema(self):
        """the shadow becomes a copy of the current parameters, the update counter 0 (e.g. after load_checkpoint)"""
        self.lib.cnnh_net_reset_ema(self.h)

    def get_ema(self):
        """the shadow arena on the host -- while swapped (swap_ema) it holds the training weights"""
        out = np.empty(self.n_params, np.float32)
        if self.lib.cnnh_net_get_ema(self.h, _fp(out)) != 0:
            raise capi.CnnAmdError("get_ema before set_ema(decay > 0)")
        return out

    def ema_updates(self):
        """updates of the average since the shadow was last (re)filled"""
        return int(self.lib.cnnh_net_ema_updates(self.h))

    def swap_ema(self):
        """Sequential::swap_ema: the arena and the shadow change places (forward, save_checkpoint, grad_cam then see the averaged
        weights); a second call, or any step, swaps back"""
        self.lib.cnnh_net_swap_ema(self.h)

    def ema_swapped(self):
        return self.lib.cnnh_net_ema_swapped(self.h) != 0

    @contextlib.contextmanager
    def averaged(self):
        """with net.averaged(): ... -- the averaged weights are swapped in for the body and swapped back on exit, also when it raises"""
        if not self.ema_swapped():
            self.swap_ema()
        try:
            yield self
        finally:
            if self.ema_swapped():
                self.swap_ema()

    def save_ema_state(self, path):
        rc = self.lib.cnnh_net_save_ema_state(self.h, str(path).encode())
        if rc != 0:
            raise capi.CnnAmdError(f"save_ema_state({path}): rc={rc}" + (" (the average was never switched on)" if rc == 4 else ""))

    def load_ema_state(self, path):
        rc = self.lib.cnnh_net_load_ema_state(self.h, str(path).encode())
        if rc == 1:
            raise FileNotFoundError(path)
        if rc != 0:
            raise capi.CnnAmdError(f"load_ema_state({path}): rc={rc}" + (" (written for another n_params)" if rc == 3 else ""))

    def save_optimizer_state(self, path):
        rc = self.lib.cnnh_net_save_optimizer_state(self.h, str(path).encode())
        if rc != 0:
            raise capi.CnnAmdError(f"save_optimizer_state({path}): rc={rc}")

    def load_optimizer_state(self, path):
        rc = self.lib.cnnh_net_load_optimizer_state(self.h, str(path).encode())
        if rc == 1:
            raise FileNotFoundError(path)
        if rc != 0:
            raise capi.CnnAmdError(f"load_optimizer_state({path}): rc={rc}" + (" (written for another n_params)" if rc == 3 else ""))

    def forward_host(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        B, _, H, W = x.shape
        out = np.empty((B, self.classes), np.float32)
        self.lib.cnnh_net_forward_host(self.h, _fp(x), B, H, W, _fp(out))
        return out

    def train_step_host(self, x, labels, lr):
        x = np.ascontiguousarray(x, dtype=np.float32)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        B, _, H, W = x.shape
        probs = np.empty((B, self.classes), np.float32)
        loss = self.lib.cnnh_net_train_step_host(self.h, _fp(x), labels.ctypes.data_as(_I), B, H, W, float(lr), _fp(probs))
        return float(loss), probs

    def train_step_device(self, x_dev, labels, lr, do_update=True):
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        B, _, H, W = x_dev.shape
        return float(self.lib.cnnh_net_train_step_device(self.h, C.c_void_p(x_dev.data_ptr()), labels.ctypes.data_as(_I), B, H,
                                                         W, float(lr), 1 if do_update else 0))

    def update(self, lr, grad_scale=1.0):
        self.lib.cnnh_net_update(self.h, float(lr), float(grad_scale))

    def train_step(self, x_dev, labels_dev, lr):
        """Sequential::train_step: forward, device-side softmax / cross-entropy, backward, [all-reduce], SGD -- nothing is read
        back and the host never blocks.  x_dev float32 [B][C][H][W], labels_dev int32 [B], both device tensors."""
        B, _, H, W = x_dev.shape
        self.lib.cnnh_net_train_step_device_loss(self.h, C.c_void_p(x_dev.data_ptr()), C.c_void_p(labels_dev.data_ptr()), B, H, W,
                                                 float(lr))

    def forward_backward(self, x_dev, labels_dev):
        """(test support) Sequential::forward_backward: train_step without its SGD step, as the plain sequence; get_grads() /
        last_loss() afterwards"""
        B, _, H, W = x_dev.shape
        self.lib.cnnh_net_forward_backward_device_loss(self.h, C.c_void_p(x_dev.data_ptr()), C.c_void_p(labels_dev.data_ptr()), B, H, W)

    def train_step_ptr(self, x_ptr, labels_dev, B, H, W, lr):
        """train_step on a raw device pointer (e.g. a capi.BatchStager slot)"""
        self.lib.cnnh_net_train_step_device_loss(self.h, C.c_void_p(x_ptr), C.c_void_p(labels_dev.data_ptr()), B, H, W, float(lr))

    def last_loss(self):
        return float(self.lib.cnnh_net_last_loss(self.h))

    def set_label_smoothing(self, eps):
        """Sequential::set_label_smoothing: every later train_step / forward_backward trains against smoothed target rows built on the
        device (cnn_soft_targets) through the soft loss head; 0 (the default) is the hard-label step, launch for launch"""
        if not 0.0 <= float(eps) < 1.0:
            raise capi.CnnAmdError(f"set_label_smoothing({eps}): eps in [0, 1)")
        self.lib.cnnh_net_set_label_smoothing(self.h, float(eps))

    def train_step_mixed(self, x_dev, labels_dev, lr, mix):
        """Sequential::train_step_mixed: cnn_batch_mix of the batch (mix: a capi.MixDesc, e.g. from mix_params) into container-owned
        storage, the mixed and smoothed targets, then the ordinary step on the mixed batch; x_dev is not written"""
        B, _, H, W = x_dev.shape
        self._mix = mix  # (kept alive across the call)
        self.lib.cnnh_net_train_step_mixed(self.h, C.c_void_p(x_dev.data_ptr()), C.c_void_p(labels_dev.data_ptr()), B, H, W, C.byref(mix), float(lr))

    def train_step_soft(self, x_dev, targets_dev, lr):
        """Sequential::train_step_soft: one step against caller-provided dense targets, float32 [B][classes] on the device"""
        B, _, H, W = x_dev.shape
        assert tuple(targets_dev.shape) == (B, self.classes) and targets_dev.is_contiguous()
        self._targets = targets_dev  # (read by the head kernel: kept alive until the next step)
        self.lib.cnnh_net_train_step_soft(self.h, C.c_void_p(x_dev.data_ptr()), C.c_void_p(targets_dev.data_ptr()), B, H, W, float(lr))

    def last_targets(self, B):
        """the [B][classes] target rows of the last soft step, on the host; synchronises"""
        out = np.empty((B, self.classes), np.float32)
        if self.lib.cnnh_net_get_targets(self.h, _fp(out), int(B)) != 0:
            raise capi.CnnAmdError("last_targets before the first step against soft targets")
        return out

    def eval_begin(self, top_k=1):
        """Sequential::eval_begin: an empty evaluation state on the device (allocated by the first call); top_k in [1, classes]"""
        if not 1 <= int(top_k) <= self.classes:
            raise capi.CnnAmdError(f"eval_begin({top_k}): top_k in [1, {self.classes}]")
        self.lib.cnnh_net_eval_begin(self.h, int(top_k))
        self._eval_begun = True

    def eval_step(self, x_dev, labels_dev):
        """Sequential::eval_step: the no-grad forward pass and ONE cnn_eval_accumulate on its logits -- loss, top-1 / top-k and confusion
        counts stay on the device, nothing is read back and the host never blocks.  x_dev float32 [B][C][H][W], labels_dev int32 [B],
        both device tensors; a label outside [0, classes), e.g. the -1 of a padded last batch, is counted as ignored only."""
        if not getattr(self, "_eval_begun", False):
            raise capi.CnnAmdError("eval_step before eval_begin")
        B, _, H, W = x_dev.shape
        self._eval_B = B
        self.lib.cnnh_net_eval_step_device(self.h, C.c_void_p(x_dev.data_ptr()), C.c_void_p(labels_dev.data_ptr()), B, H, W)

    def eval_result(self):
        """Sequential::eval_result: the totals since eval_begin -- the one read-back, synchronises.  A dict of samples, top1, topk,
        ignored, loss_sum, mean_loss, accuracy (NaN without samples) and confusion (numpy uint64 [classes][classes], row = label,
        column = prediction)"""
        if not getattr(self, "_eval_begun", False):
            raise capi.CnnAmdError("eval_result before eval_begin")
        res = capi.EvalResult()
        conf = np.zeros((self.classes, self.classes), np.uint64)
        self.lib.cnnh_net_eval_result(self.h, C.byref(res), conf.ctypes.data_as(C.c_void_p))
        n = int(res.samples)
        return {"samples": n, "top1": int(res.top1), "topk": int(res.topk), "ignored": int(res.ignored), "loss_sum": float(res.loss_sum),
                "mean_loss": float(res.loss_sum) / n if n else float("nan"), "accuracy": int(res.top1) / n if n else float("nan"),
                "confusion": conf}

    def predictions(self):
        """the int32 predictions of the last eval_step, on the host; synchronises"""
        B = getattr(self, "_eval_B", 0)
        out = np.empty(B, np.int32)
        if B == 0 or self.lib.cnnh_net_get_predictions(self.h, out.ctypes.data_as(_I), B) != 0:
            raise capi.CnnAmdError("predictions before the first eval_step")
        return out

    def evaluate(self, batches, top_k=1):
        """eval_begin, one eval_step per (x_dev, labels_dev) of the iterable, eval_result"""
        self.eval_begin(top_k)
        for x_dev, labels_dev in batches:
            self.eval_step(x_dev, labels_dev)
        return self.eval_result()

    def train_step_ptrs(self, x_ptr, labels_ptr, B, H, W, lr):
        """train_step on two raw device pointers (a resident capi.BatchStager's submit() and labels(slot))"""
        self.lib.cnnh_net_train_step_device_loss(self.h, C.c_void_p(x_ptr), C.c_void_p(labels_ptr), int(B), int(H), int(W), float(lr))

    def eval_step_ptrs(self, x_ptr, labels_ptr, B, H, W):
        """eval_step on two raw device pointers"""
        if not getattr(self, "_eval_begun", False):
            raise capi.CnnAmdError("eval_step_ptrs before eval_begin")
        self._eval_B = int(B)
        self.lib.cnnh_net_eval_step_device(self.h, C.c_void_p(x_ptr), C.c_void_p(labels_ptr), int(B), int(H), int(W))

    def _resident_loop(self, stager, order, params, step):
        """one pass over the rows of `order` through a resident stager with one batch of look-ahead: batch i + 1 is submitted (its
        gather runs on the stager's stream) before batch i is stepped on the current stream; step(x_ptr, labels_ptr, B, H, W)"""
        B, H, W = stager.B, stager.H, stager.W

        def submit(row):
            _, slot = stager.acquire()
            stager.indices(slot)[:] = row
            if params is not None:
                mats, blocks = params(row)
                if mats is not None:
                    stager.matrices(slot)[:] = mats
                if blocks is not None:
                    stager.photo(slot)[:] = blocks
            return slot, stager.submit(slot)

        ahead = submit(order[0]) if len(order) else None
        for i in range(len(order)):
            slot, x_ptr = ahead
            ahead = submit(order[i + 1]) if i + 1 < len(order) else None
            stager.wait(slot)
            step(x_ptr, stager.labels(slot), B, H, W)
            stager.release(slot)

    @staticmethod
    def _resident_order(stager, order, what):
        order = np.ascontiguousarray(order, dtype=np.int32)
        if getattr(stager, "resident", None) is None:
            raise capi.CnnAmdError(f"{what}: the stager is not a resident one (capi.BatchStager(u8_shape=..., resident=ds))")
        if order.ndim != 2 or order.shape[1] != stager.B:
            raise capi.CnnAmdError(f"{what}: order must be int32 [steps][{stager.B}] (hostapi.epoch_order)")
        n = stager.resident.N
        if order.size and (int(order.min()) < -1 or int(order.max()) >= n):
            raise capi.CnnAmdError(f"{what}: an index outside [-1, {n})")
        return order

    def train_epoch_resident(self, stager, order, lr, params=None):
        """One epoch out of a resident dataset: per row of `order` (int32 [steps][B], hostapi.epoch_order(..., drop_last=True)) the
        stager gathers the batch and its labels on the device and train_step runs on them;
        params(row) -> (matrices (B, 6) or None, photo blocks (B, 20) or None) is written into the slot when given.  An order that
        contains -1 is refused before anything is enqueued: the training loss head indexes its row by the label, and the -1 of a padded
        row would be an access out of bounds, not an ignored sample.  A stager of depth 3 keeps the host ahead: with two slots the
        acquire() for batch i + 1 waits for step i - 1 to finish, and step i is queued only behind that wait (correct, 4 % slower:
        profiles/resident_dataset.md)."""
        order = self._resident_order(stager, order, "train_epoch_resident")
        if order.size and int(order.min()) < 0:
            raise capi.CnnAmdError("train_epoch_resident: the order contains -1 (a padded row); train with epoch_order(..., drop_last=True)")
        self._resident_loop(stager, order, params, lambda x, l, B, H, W: self.train_step_ptrs(x, l, B, H, W, lr))

    def evaluate_resident(self, stager, order, top_k=1):
        """evaluate() out of a resident dataset: eval_begin, one eval_step per row of `order`, eval_result.  The -1 of a padded last
        row is right here: its sample is a fill image with label -1, which cnn_eval_accumulate counts as ignored and nowhere else."""
        order = self._resident_order(stager, order, "evaluate_resident")
        self.eval_begin(top_k)
        self._resident_loop(stager, order, None, self.eval_step_ptrs)
        return self.eval_result()

    def input_delta(self, shape):
        """the delta with respect to the network input of the last backward pass (the first layer's data gradient)"""
        out = np.empty(shape, np.float32)
        rc = self.lib.cnnh_net_input_delta(self.h, _fp(out), out.size)
        if rc != 0:
            raise KeyError(f"input_delta: rc={rc}")
        return out

    def flush(self):
        """Sequential::flush_deferred(): the data gradient train_step deferred into the next pass is launched / ordered now"""
        self.lib.cnnh_net_flush(self.h)

    def layer_output(self, name, shape):
        out = np.empty(shape, np.float32)
        rc = self.lib.cnnh_net_layer_output(self.h, name.encode(), _fp(out), out.size)
        if rc == 3:  # std::runtime_error from Layer::get_output(): the tensor was fused away and its parameters are gone
            raise RuntimeError(f"layer {name}: get_output() of a tensor the last forward pass did not write, after its parameters were overwritten")
        if rc != 0:
            raise KeyError(f"layer {name}: rc={rc}")
        return out


    def grad_cam(self, layer_name, shape):
        """Sequential::grad_cam (alexnet.cpp:95-142) after a forward pass with gradients enabled; shape = (B, H, W) of the layer's
        feature map.  Returns (uint8 image [H][W] -- the reference's cv::Mat --, normalised cam [B][H][W])"""
        B, H, W = shape
        img = np.empty((H, W), np.uint8)
        cam = np.empty((B, H, W), np.float32)
        rc = self.lib.cnnh_net_grad_cam(self.h, layer_name.encode(), img.ctypes.data_as(C.c_void_p), img.size, _fp(cam), cam.size)
        if rc != 0:
            raise KeyError(f"grad_cam({layer_name}): rc={rc}")
        return img, cam


class HostAlexNet(HostNet):
    """architectures::AlexNet: the reference's fixed list (alexnet.cpp:10-33)"""

    def __init__(self, classes=3, params=None, grads=None, batch_norm=False):
        self.lib = load()
        p = C.c_void_p(params.data_ptr()) if params is not None else None
        g = C.c_void_p(grads.data_ptr()) if grads is not None else None
        self._adopt(self.lib.cnnh_net_create_ex(classes, p, g, 1 if batch_norm else 0), classes, params, grads)


def _layer_names(spec):
    """the naming scheme of sequential.cpp's StackBuilder / the reference (conv_layer_N, bn_layer_N, relu_layer_N, max_pool_N)"""
    names, n_conv, n_pool, n_lin = [], 0, 0, 0
    for item in spec:
        kind = item[0]
        if kind == "conv":
            n_conv += 1
            names.append(f"conv_layer_{n_conv}")
        elif kind == "dwconv":  # (counted with the convolutions: the layers behind it carry its number)
            n_conv += 1
            names.append(f"dw_layer_{n_conv}")
        elif kind == "bn":
            names.append(f"bn_layer_{n_conv}")
        elif kind == "relu":
            names.append(f"relu_layer_{n_conv}")
        elif kind == "pool":
            n_pool += 1
            names.append(f"max_pool_{n_pool}")
        elif kind == "dropout":
            names.append(f"dropout_layer_{n_conv}")
        else:
            n_lin += 1
            names.append(f"linear_{n_lin}")
    return names


class HostSequential(HostNet):
    """architectures::Sequential built from a cnn_amd.stacks spec (any list of the reference's layer types)"""

    def __init__(self, spec, in_shape=(3, 224, 224), params=None, grads=None):
        from . import stacks

        self.lib = load()
        self.spec = list(spec)
        self.layout = stacks.walk(self.spec, *in_shape)
        self.names = _layer_names(self.spec)
        classes = self.layout[-1]["out"][0]
        h = C.c_void_p(self.lib.cnnh_seq_create(in_shape[0], classes))
        for name, item, ent in zip(self.names, self.spec, self.layout):
            nm = name.encode()
            if item[0] == "conv":
                self.lib.cnnh_seq_add_conv(h, nm, ent["in"][0], item[1], item[2], item[3], item[4])
            elif item[0] == "dwconv":
                self.lib.cnnh_seq_add_dwconv(h, nm, ent["in"][0], item[1], item[2], item[3])
            elif item[0] == "bn":
                self.lib.cnnh_seq_add_bn(h, nm, ent["in"][0])
            elif item[0] == "relu":
                self.lib.cnnh_seq_add_relu(h, nm)
            elif item[0] == "pool":
                self.lib.cnnh_seq_add_pool(h, nm, item[1], item[2])
            elif item[0] == "dropout":
                self.lib.cnnh_seq_add_dropout(h, nm, float(item[1]))
            else:
                self.lib.cnnh_seq_add_linear(h, nm, ent["n_in"], ent["n_out"])
        p = C.c_void_p(params.data_ptr()) if params is not None else None
        g = C.c_void_p(grads.data_ptr()) if grads is not None else None
        self.lib.cnnh_seq_finalize(h, p, g)
        self._adopt(h.value, classes, params, grads)
        assert self.n_params == sum(e["params"] for e in self.layout)


class HostStack(HostNet):
    """architectures::build_vgg11 / build_resnet18 (sequential.cpp) -- the C++ side's own builders of the BASELINE stacks"""

    def __init__(self, which, classes=3, batch_norm=False):
        self.lib = load()
        h = self.lib.cnnh_stack_create(which.encode(), classes, 1 if batch_norm else 0)
        if not h:
            raise KeyError(which)
        hh = C.c_void_p(h)
        self.lib.cnnh_seq_finalize(hh, None, None)
        self._adopt(h, classes, None, None)
