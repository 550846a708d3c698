"""Host-side mirror of the reference's main() (resnet.cu:3222-3429) over the C-ABI: same call
sequence (init_dimensions -> init_resnet -> init_general_batch -> init_trainer, then per step
load_new_batch -> forward_pass -> host loss -> backwards_pass -> update_parameters)."""
import ctypes as C

import numpy as np

from . import binding as B


def resnet_dims(input=224, n_conv_blocks=16, reductions=(3, 7, 13), final_depth=2048, output=1000,
                init_conv_filters=64):
    """the literals of resnet.cu:3245-3258"""
    return dict(input=input, init_kernel_dim=7, init_conv_filters=init_conv_filters, init_conv_stride=2,
                init_maxpool_dim=3, init_maxpool_stride=2, n_conv_blocks=n_conv_blocks,
                is_block_spatial_reduction=[1 if i in reductions else 0 for i in range(n_conv_blocks)],
                final_depth=final_depth, output=output)


class Trainer:
    def __init__(self, dims, batch, lr=1e-4, wd=0.0, b1=0.9, b2=0.999, eps=1e-7, seed=1234, n_epochs=1,
                 dump_dir="default", shard_n_images=None, device=None):
        self.L = L = B.load()
        if device is not None:
            if L.mi_set_device(int(device)) != 0:
                raise RuntimeError(self.error())
        self.dims, self.batch = dict(dims), batch
        nb = dims["n_conv_blocks"]
        self._flags = (C.c_int * max(nb, 1))(*dims["is_block_spatial_reduction"])
        self.c_dims = L.init_dimensions(dims["input"], dims["init_kernel_dim"], dims["init_conv_filters"],
                                        dims["init_conv_stride"], dims["init_maxpool_dim"], dims["init_maxpool_stride"],
                                        nb, self._flags, dims["final_depth"], dims["output"])
        rng = L.mi_rng_create(seed)
        self.model = L.init_resnet(self.c_dims, rng)
        L.mi_rng_destroy(rng)
        image_size = dims["input"] * dims["input"] * 3
        self.c_batch = L.init_general_batch(batch, image_size, dims["input"], shard_n_images or batch)
        self._dump_dir = dump_dir.encode()
        self.t = L.init_trainer(self.model, self.c_batch, batch, lr, wd, b1, b2, eps, n_epochs, self._dump_dir)
        self.check()
        p = self.t.contents.model.contents.params.contents
        self.n_locations = p.n_locations
        self.sizes = [p.sizes[i] for i in range(p.n_locations)]
        L.mi_trainer_set_dump_every(self.t, 0)
        self.dtype = B.MI_DTYPE_F32

    # ---- options (before the first step) ----
    def set_dtype(self, dtype):
        """MI_DTYPE_BF16: activations / activation gradients stored as bf16 (BASELINE configs[4])"""
        if self.L.mi_trainer_set_dtype(self.t, int(dtype)) != 0:
            e = self.error()
            self.L.mi_clear_error()
            raise RuntimeError("mi_trainer_set_dtype: " + e)
        self.dtype = int(dtype)

    OPTIMIZERS = {"adam": B.MI_OPT_ADAM, "sgd": B.MI_OPT_SGD, "lars": B.MI_OPT_LARS}

    def set_optimizer(self, kind, momentum=0.9, trust=0.001):
        """"adam" (the reference's, default), "sgd" (momentum SGD) or "lars"; before the first update (include/resnet_mi.h)"""
        if self.L.mi_trainer_set_optimizer(self.t, self.OPTIMIZERS[kind], momentum, trust) != 0:
            e = self.error()
            self.L.mi_clear_error()
            raise RuntimeError("mi_trainer_set_optimizer: " + e)

    def optimizer(self):
        return {v: k for k, v in self.OPTIMIZERS.items()}[self.L.mi_trainer_get_optimizer(self.t)]

    def set_loss(self, smoothing=0.0, topk=5, device=True, copy_pred=True):
        """the head of forward / backward (mi_trainer_set_loss, include/resnet_mi.h).  device: soft-max, label-smoothed cross-entropy
        gradient, loss and top-1 / top-k totals in one launch on the GPU (metrics()); copy_pred=False also drops forward()'s blocking
        copy of pred to the host, loss() then reads the device's record.  device=False, smoothing 0: the reference's head"""
        flags = (B.MI_LOSS_DEVICE if device else 0) | (0 if copy_pred else B.MI_LOSS_NO_PRED_COPY)
        if self.L.mi_trainer_set_loss(self.t, smoothing, int(topk), flags) != 0:
            e = self.error()
            self.L.mi_clear_error()
            raise RuntimeError("mi_trainer_set_loss: " + e)

    def metrics(self, reset=False):
        """(last, total): loss_sum, rows, wrong_top1, wrong_topk, batches of the last forward() and summed since the last reset"""
        last, total = B.MiLossMetrics(), B.MiLossMetrics()
        if self.L.mi_trainer_metrics(self.t, C.byref(last), C.byref(total), int(bool(reset))) != 0:
            raise RuntimeError("mi_trainer_metrics: " + self.error())
        return last.as_dict(), total.as_dict()

    # ---- evaluation (include/resnet_mi.h, "evaluation") ----
    def _refused(self, what):
        e = self.error()
        self.L.mi_clear_error()
        raise RuntimeError(what + ": " + e)

    # ---- mixing (include/resnet_mi.h, "mixing") ----
    def set_mix(self, mixup=0.2, cutmix=1.0, prob=1.0, switch=0.5, seed=0):
        """mixup / CutMix on the device at every load_new_batch (row i with row batch - 1 - i) and the two-label loss head in forward();
        needs set_loss(device=True) first.  mixup, cutmix: the Beta(alpha, alpha) parameters in (0, 1], 0 = that mode off (both 0: mixing
        off); prob: the share of steps that mix; switch: the share of CutMix among them when both are on"""
        if self.L.mi_trainer_set_mix(self.t, float(mixup), float(cutmix), float(prob), float(switch), int(seed)) != 0:
            self._refused("mi_trainer_set_mix")

    def last_mix(self):
        """the plan of the last load_new_batch as a dict: mode (0 none, 1 mixup, 2 CutMix), lam, y0, x0, y1, x1"""
        p = B.MiMixPlan()
        if self.L.mi_trainer_last_mix(self.t, C.byref(p)) != 0:
            self._refused("mi_trainer_last_mix")
        return p.as_dict()

    # ---- random erasing (include/resnet_mi.h, "random erasing") ----
    def set_erase(self, prob=0.1, scale=(0.02, 0.33), ratio=(0.3, 3.3), mode="const", value=(0, 0, 0), std=(58.395, 57.12, 57.375), seed=0):
        """random erasing on the device at every load_new_batch, in front of the mix step: with probability prob a row gets one box of
        scale[0] .. scale[1] of the image's area and aspect ratio[0] .. ratio[1] (torchvision's RandomErasing), filled with value per
        plane (mode "const") or with value + std z, z nearly normal (mode "noise", timm's pixel mode).  The images are mean-subtracted
        but not divided: value 0 is the mean pixel, as it is behind torchvision's Normalize, and the default std is ImageNet's in byte
        units.  prob 0: off"""
        fill = B.erase_fill_struct(mode, value, std)
        if self.L.mi_trainer_set_erase(self.t, float(prob), float(scale[0]), float(scale[1]), float(ratio[0]), float(ratio[1]), C.byref(fill),
                                       int(seed) & (2 ** 64 - 1)) != 0:
            self._refused("mi_trainer_set_erase")

    def last_erase(self):
        """the boxes of the last load_new_batch: int32 (rows, 4), a row (y0, x0, h, w); h == 0 or w == 0: that row was not erased"""
        out = np.zeros((self.batch, 4), np.int32)
        rows = self.L.mi_trainer_last_erase(self.t, out.ctypes.data)
        if rows < 0:
            self._refused("mi_trainer_last_erase")
        return out[:rows]

    # ---- TrivialAugmentWide (include/resnet_mi.h, "TrivialAugmentWide") ----
    def set_trivial_augment(self, seed=0, on=True):
        """TrivialAugmentWide on the device at every load_new_batch, in front of the erase and mix steps (torchvision's --auto-augment
        ta_wide): per row one of 14 Pillow operations at one of 31 strengths, Pillow's bytes bit for bit"""
        if self.L.mi_trainer_set_trivial_augment(self.t, 1 if on else 0, int(seed) & (2 ** 64 - 1)) != 0:
            self._refused("mi_trainer_set_trivial_augment")

    def last_trivial_augment(self):
        """the records of the last load_new_batch: a list of dicts (op, bin, neg, arg, magnitude, factor, A)"""
        out = (B.MiTaRow * self.batch)()
        rows = self.L.mi_trainer_last_trivial_augment(self.t, out)
        if rows < 0:
            self._refused("mi_trainer_last_trivial_augment")
        return [out[i].as_dict() for i in range(rows)]

    def track_running_stats(self, momentum=0.1, on=True):
        """keep torch.nn.BatchNorm2d's running statistics of every batch norm: one extra launch per forward(); after set_dtype, before
        the first forward()"""
        if self.L.mi_trainer_track_running_stats(self.t, int(bool(on)), float(momentum)) != 0:
            self._refused("mi_trainer_track_running_stats")

    def running_stats(self):
        """(means, vars): float32 arrays over every BN layer's channels, the layers in the order of their gammas in locations[]"""
        n = self.L.mi_trainer_running_stats_channels(self.t)
        means, vars_ = np.empty(n, np.float32), np.empty(n, np.float32)
        if self.L.mi_trainer_get_running_stats(self.t, means.ctypes.data, vars_.ctypes.data) != 0:
            self._refused("mi_trainer_get_running_stats")
        return means, vars_

    def set_running_stats(self, means, vars):
        n = self.L.mi_trainer_running_stats_channels(self.t)
        means, vars = np.ascontiguousarray(means, np.float32).ravel(), np.ascontiguousarray(vars, np.float32).ravel()
        if n and (means.size != n or vars.size != n):
            raise ValueError("running statistics hold %d channels" % n)
        if self.L.mi_trainer_set_running_stats(self.t, means.ctypes.data, vars.ctypes.data) != 0:
            self._refused("mi_trainer_set_running_stats")

    def running_updates(self):
        return int(self.L.mi_trainer_running_updates(self.t))

    def eval_forward(self, images=None, labels=None, n_valid=None, topk=5):
        """the eval pass (running statistics, nothing trained): on the current batch, or on images (NCHW float32, up to `batch` of them;
        missing rows are zero) and labels copied to the device.  Metrics over the first n_valid rows: eval_metrics()"""
        b = self.c_batch.contents
        if images is None:
            im, lab = C.cast(b.images, C.c_void_p), C.cast(b.correct_classes, C.c_void_p)
            n_valid = self.batch if n_valid is None else n_valid
        else:
            d = self.dims["input"]
            images = np.ascontiguousarray(images, np.float32).reshape(-1, 3, d, d)
            if images.shape[0] > self.batch:
                raise ValueError("more images than the batch size")
            n_valid = images.shape[0] if n_valid is None else n_valid
            full = np.zeros((self.batch, 3, d, d), np.float32)
            full[:images.shape[0]] = images
            im, lab = self._eval_dev("_eval_images_dev", full.nbytes), None
            self.L.mi_copy_to_device(im, full.ctypes.data, full.nbytes)
            if labels is not None:
                lab_h = np.zeros(self.batch, np.int32)
                lab_h[:len(labels)] = np.asarray(labels, np.int32)
                lab = self._eval_dev("_eval_labels_dev", lab_h.nbytes)
                self.L.mi_copy_to_device(lab, lab_h.ctypes.data, lab_h.nbytes)
        if self.L.mi_trainer_eval_forward(self.t, im, lab, int(n_valid), int(topk)) != 0:
            self._refused("mi_trainer_eval_forward")

    def _eval_dev(self, name, nbytes):
        """a device buffer of eval_forward's own, made once"""
        if not getattr(self, name, None):
            p = self.L.mi_malloc(nbytes)
            if not p:
                raise MemoryError("mi_malloc(%d)" % nbytes)
            setattr(self, name, p)
        return getattr(self, name)

    def eval_metrics(self, reset=False):
        """(last, total) of the eval passes, as metrics()"""
        last, total = B.MiLossMetrics(), B.MiLossMetrics()
        if self.L.mi_trainer_eval_metrics(self.t, C.byref(last), C.byref(total), int(bool(reset))) != 0:
            self._refused("mi_trainer_eval_metrics")
        return last.as_dict(), total.as_dict()

    def evaluate_u8(self, images_u8, labels, dim_in, topk=5, resize=None):
        """a whole array of dim_in x dim_in x 3 (B,G,R) byte images: centre crop, decode and eval pass per batch on the device; the
        totals as a dict (loss_sum, rows, wrong_top1, wrong_topk, batches).  resize: every image is first scaled to resize x resize as
        Pillow's BILINEAR does (antialiased) and the centre crop is taken from that (mi_trainer_eval_u8_resized)"""
        images_u8 = np.ascontiguousarray(images_u8, np.uint8)
        labels = np.ascontiguousarray(labels, np.int32)
        n = labels.size
        if images_u8.size != n * dim_in * dim_in * 3:
            raise ValueError("images_u8 does not hold %d images of %d x %d x 3 bytes" % (n, dim_in, dim_in))
        out = B.MiLossMetrics()
        if resize is not None:
            if self.L.mi_trainer_eval_u8_resized(self.t, images_u8.ctypes.data, labels.ctypes.data, n, int(dim_in), int(resize), int(topk),
                                                 C.byref(out)) != 0:
                self._refused("mi_trainer_eval_u8_resized")
        elif self.L.mi_trainer_eval_u8(self.t, images_u8.ctypes.data, labels.ctypes.data, n, int(dim_in), int(topk), C.byref(out)) != 0:
            self._refused("mi_trainer_eval_u8")
        return out.as_dict()

    # ---- weight averaging (include/resnet_mi.h, "weight averaging") ----
    def set_ema(self, decay=0.9999, every=1, warmup=False):
        """keep an exponential moving average of the parameters and the BN running statistics on the device: e <- lerp(e, p, 1 - decay)
        behind every `every`-th update() (0: updates off, values kept); warmup: timm's min(decay, (1 + k) / (10 + k)).  The first call
        takes a snapshot of the current values; needs track_running_stats() first"""
        if self.L.mi_trainer_set_ema(self.t, float(decay), int(every), int(bool(warmup))) != 0:
            self._refused("mi_trainer_set_ema")

    def ema_reset(self):
        """the snapshot again, update counter 0"""
        if self.L.mi_trainer_ema_reset(self.t) != 0:
            self._refused("mi_trainer_ema_reset")

    def ema_updates(self):
        return int(self.L.mi_trainer_ema_updates(self.t))

    def ema_get(self, i):
        out = np.empty(self.sizes[i] if 0 <= i < self.n_locations else 1, np.float32)
        if self.L.mi_trainer_ema_get_location(self.t, int(i), out.ctypes.data) != 0:
            self._refused("mi_trainer_ema_get_location")
        return out

    def ema_set(self, i, arr):
        arr = np.ascontiguousarray(arr, np.float32).ravel()
        if 0 <= i < self.n_locations and arr.size != self.sizes[i]:
            raise ValueError("location %d holds %d floats" % (i, self.sizes[i]))
        if self.L.mi_trainer_ema_set_location(self.t, int(i), arr.ctypes.data) != 0:
            self._refused("mi_trainer_ema_set_location")

    def ema_running_stats(self):
        """(means, vars) of the averaged model, as running_stats()"""
        n = self.L.mi_trainer_running_stats_channels(self.t)
        means, vars_ = np.empty(n, np.float32), np.empty(n, np.float32)
        if self.L.mi_trainer_ema_get_running_stats(self.t, means.ctypes.data, vars_.ctypes.data) != 0:
            self._refused("mi_trainer_ema_get_running_stats")
        return means, vars_

    def set_ema_running_stats(self, means, vars):
        n = self.L.mi_trainer_running_stats_channels(self.t)
        means, vars = np.ascontiguousarray(means, np.float32).ravel(), np.ascontiguousarray(vars, np.float32).ravel()
        if n and (means.size != n or vars.size != n):
            raise ValueError("running statistics hold %d channels" % n)
        if self.L.mi_trainer_ema_set_running_stats(self.t, means.ctypes.data, vars.ctypes.data) != 0:
            self._refused("mi_trainer_ema_set_running_stats")

    def eval_use_ema(self, on=True):
        """while on, eval_forward() and evaluate_u8() score the averaged model (the arenas are exchanged around the pass, on the device)"""
        if self.L.mi_trainer_eval_use_ema(self.t, int(bool(on))) != 0:
            self._refused("mi_trainer_eval_use_ema")

    # ---- gradient accumulation (include/resnet_mi.h, "gradient accumulation") ----
    def set_accumulation(self, k, scale=1.0):
        """k micro-batches per optimizer update: of every k update() calls the first k - 1 only sum the gradient arena on the device, the
        k-th applies (sum * scale) through the optimizer once (scale 1 / k: the mean over micro-batches).  step() stays one micro-batch.
        Between windows only; k = 1: off"""
        if self.L.mi_trainer_set_accumulation(self.t, int(k), float(scale)) != 0:
            self._refused("mi_trainer_set_accumulation")

    def accumulation(self):
        """(k, pending): the setting and the micro-batches summed so far in this window"""
        k, pending = C.c_int(0), C.c_int(0)
        if self.L.mi_trainer_accumulation(self.t, C.byref(k), C.byref(pending)) != 0:
            self._refused("mi_trainer_accumulation")
        return k.value, pending.value

    # ---- gradient clipping, norm weight decay (include/resnet_mi.h, "gradient clipping") ----
    def set_clip_grad_norm(self, max_norm):
        """clip the gradient the optimizer sees to a global L2 norm of max_norm at every applied update(), on the device (torchvision's
        --clip-grad-norm; the gradient is a batch sum); 0: off.  Between updates only"""
        if self.L.mi_trainer_set_clip_grad_norm(self.t, float(max_norm)) != 0:
            self._refused("mi_trainer_set_clip_grad_norm")

    def last_clip(self):
        """the record of the last clipped update as a dict: sq_norm, norm (before scaling: what torch's clip_grad_norm_ returns), coef,
        nonfinite, and the running counters updates and clipped"""
        r = B.MiClipRecord()
        if self.L.mi_trainer_last_clip(self.t, C.byref(r)) != 0:
            self._refused("mi_trainer_last_clip")
        return r.as_dict()

    def set_norm_weight_decay(self, wd):
        """SGD only: BN gamma / beta decay with wd in place of the trainer's weight decay (torchvision's --norm-weight-decay)"""
        if self.L.mi_trainer_set_norm_weight_decay(self.t, float(wd)) != 0:
            self._refused("mi_trainer_set_norm_weight_decay")

    def set_lr(self, lr):
        """learning_rate for the next update_parameters and on (read at every update)"""
        self.t.contents.learning_rate = lr

    def set_store_policy(self, policy):
        if self.L.mi_trainer_set_store_policy(self.t, int(policy)) != 0:
            e = self.error()
            self.L.mi_clear_error()
            raise RuntimeError("mi_trainer_set_store_policy: " + e)

    def activation_bytes(self):
        return int(self.L.mi_trainer_activation_bytes(self.t))

    def device_bytes(self):
        return int(self.L.mi_trainer_device_bytes(self.t))

    def check_errors(self):
        return int(self.L.mi_trainer_check_errors(self.t))

    # ---- plumbing ----
    def error(self):
        return self.L.mi_last_error().decode()

    def check(self):
        e = self.error()
        if e:
            raise RuntimeError("libresnet_mi: " + e)

    def close(self):
        if self.t:
            self.L.destroy_trainer(self.t)
            self.t = None
            for name in ("_eval_images_dev", "_eval_labels_dev"):
                if getattr(self, name, None):
                    self.L.mi_free(getattr(self, name))
                    setattr(self, name, None)

    def _to_host(self, ptr, n, dtype=np.float32):
        out = np.empty(n, dtype)
        self.L.mi_copy_to_host(out.ctypes.data, C.cast(ptr, C.c_void_p), n * 4)
        return out

    def _act_to_host(self, ptr, n):
        """an activation-typed tensor (bf16 in bf16 mode) widened to float32"""
        if self.dtype == B.MI_DTYPE_F32:
            return self._to_host(ptr, n)
        raw = np.empty(n, np.uint16)
        self.L.mi_copy_to_host(raw.ctypes.data, C.cast(ptr, C.c_void_p), n * 2)
        return (raw.astype(np.uint32) << 16).view(np.float32)

    def _to_dev(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        self.L.mi_copy_to_device(C.cast(ptr, C.c_void_p), arr.ctypes.data, arr.nbytes)

    def _pset(self, which):
        t = self.t.contents
        if which == "params":
            return t.model.contents.params.contents
        bb = t.backprop_buffer.contents
        return {"grads": bb.param_derivs, "means": bb.prev_means, "vars": bb.prev_vars}[which].contents

    def get(self, which, i):
        p = self._pset(which)
        return self._to_host(p.locations[i], p.sizes[i])

    def set(self, which, i, arr):
        p = self._pset(which)
        assert arr.size == p.sizes[i]
        self._to_dev(p.locations[i], arr.astype(np.float32).ravel())

    def set_params(self, arrays):
        for i, a in enumerate(arrays):
            self.set("params", i, a)

    # ---- data sources ----
    def source_synthetic(self, seed_images=1234, seed_labels=1235, pool_batches=2):
        self.L.mi_batch_source_synthetic(self.c_batch, seed_images, seed_labels, self.dims["output"], pool_batches)
        self.check()

    def source_host(self, layout=B.MI_LAYOUT_NHWC):
        self.L.mi_batch_source_host(self.c_batch, layout)

    def source_buffer(self, images_path, labels_path, layout=B.MI_LAYOUT_NHWC):
        self.L.mi_batch_source_buffer(self.c_batch, images_path.encode(), labels_path.encode(), layout)

    def source_shards(self, shard_dir, layout=B.MI_LAYOUT_NCHW, prefetch=False):
        self.L.mi_batch_source_shards(self.c_batch, shard_dir.encode(), layout)
        if prefetch:
            self.L.mi_batch_set_prefetch(self.c_batch, 1)

    AUGMENTS = {"fixed": B.MI_AUG_FIXED, "center": B.MI_AUG_CENTER, "random": B.MI_AUG_RANDOM, "rrc": B.MI_AUG_RRC}

    def source_shards_u8(self, shard_dir, dim_in, augment="fixed", flip=True, seed=0, prefetch=False, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3),
                         antialias=False):
        """uint8 shards of whole dim_in x dim_in images (mi_build_shard_u8); crop, flip and float conversion on the device at
        every load.  augment: "fixed" (the shard's .crops, the reference's pixels), "center", "random" (a new draw per epoch) or "rrc"
        (random-resized crop: a box of `scale` of the image's area and aspect `ratio`, resampled to the input size; a new draw per epoch).
        antialias: the "rrc" boxes are scaled as Pillow's BILINEAR scales them (the filter widened by the scale factor), not by the
        two-tap gather"""
        self.L.mi_batch_source_shards_u8(self.c_batch, shard_dir.encode(), int(dim_in))
        if self.AUGMENTS[augment] == B.MI_AUG_RRC:
            rc, what = self.L.mi_batch_set_augment_rrc(self.c_batch, int(bool(flip)), int(seed), float(scale[0]), float(scale[1]),
                                                       float(ratio[0]), float(ratio[1])), "mi_batch_set_augment_rrc: "
        else:
            rc, what = self.L.mi_batch_set_augment(self.c_batch, self.AUGMENTS[augment], int(bool(flip)), int(seed)), "mi_batch_set_augment: "
        if rc != 0:
            e = self.error()
            self.L.mi_clear_error()
            raise RuntimeError(what + e)
        self.L.mi_batch_set_antialias(self.c_batch, int(bool(antialias)))
        if prefetch:
            self.L.mi_batch_set_prefetch(self.c_batch, 1)
        self.check()

    def last_plan(self):
        """(row_off, col_off, flip) per image of the last load_new_batch (uint8 shards), int32 (batch, 3)"""
        out = np.empty((self.batch, 3), np.int32)
        if self.L.mi_batch_last_plan(self.c_batch, out.ctypes.data) != self.batch:
            raise RuntimeError("no plan: the source is not uint8 shards, the mode is rrc (last_boxes), or nothing was loaded yet")
        return out

    def last_boxes(self):
        """(row0, col0, box_h, box_w, flip) per image of the last load_new_batch (uint8 shards, augment="rrc"), int32 (batch, 5)"""
        out = np.empty((self.batch, 5), np.int32)
        if self.L.mi_batch_last_boxes(self.c_batch, out.ctypes.data) != self.batch:
            raise RuntimeError("no boxes: the source is not uint8 shards in rrc mode, or nothing was loaded yet")
        return out

    def fill_host_batch(self, images, labels):
        """write the caller-owned pinned staging buffers (images_float_cpu / correct_classes_cpu)"""
        b = self.c_batch.contents
        n = b.n_images * b.image_size
        np.ctypeslib.as_array(b.images_float_cpu, shape=(n,))[:] = np.ascontiguousarray(images, np.float32).ravel()
        np.ctypeslib.as_array(b.correct_classes_cpu, shape=(b.n_images,))[:] = np.asarray(labels, np.int32)

    # ---- the reference main loop, one call each ----
    def load_new_batch(self):
        self.L.load_new_batch(self.t, None, self.c_batch)

    def forward(self):
        self.L.forward_pass(self.t)

    def loss(self):
        nw = C.c_int(0)
        return float(self.L.mi_host_loss(self.t, C.byref(nw))), nw.value

    def backward(self):
        self.L.backwards_pass(self.t)

    def update(self):
        self.L.update_parameters(self.t)

    def step(self):
        self.load_new_batch()
        self.forward()
        loss = self.loss()
        self.backward()
        self.update()
        return loss

    def pred(self):
        t = self.t.contents
        n = self.batch * self.dims["output"]
        return np.ctypeslib.as_array(t.forward_buffer.contents.pred_cpu, shape=(n,)).reshape(self.batch, -1).copy()

    def stem_dtype(self):
        """storage type of the stem convolution's own output and its gradient (MI_DTYPE_*)"""
        return self.L.mi_trainer_stem_dtype(self.t)

    def routes(self):
        """(fwd, dgrad, wgrad, fz) of every convolution of the trainer's table (mi_layer_routes' numbers): the stem, then per block the
        reduction, the spatial convolution, the expansion and the projection where the block has one"""
        n = self.L.mi_debug_trainer_routes(self.t, None, 0)
        out = (C.c_int * (4 * n))()
        assert self.L.mi_debug_trainer_routes(self.t, out, 4 * n) == n
        return [tuple(out[4 * i:4 * i + 4]) for i in range(n)]

    def labels(self):
        return np.ctypeslib.as_array(self.c_batch.contents.correct_classes_cpu, shape=(self.batch,)).copy()

    def timings(self):
        out = (C.c_float * 5)()
        self.L.mi_trainer_last_timings(self.t, C.byref(out))
        return list(out)

    # ---- activation access by the reference's dump names (NCHW arrays) ----
    def activation(self, name, deriv=False):
        t = self.t.contents
        a = (t.backprop_buffer.contents.activation_derivs if deriv else t.forward_buffer.contents.activations).contents
        d, N = self.dims, self.batch
        f = d["init_conv_filters"]
        Hs = d["input"] // d["init_conv_stride"]
        Hp = Hs // d["init_maxpool_stride"]
        if name == "input":
            return self._to_host(self.c_batch.contents.images, N * 3 * d["input"] ** 2).reshape(N, 3, d["input"], d["input"])
        if name == "init_conv_applied":  # the stem convolution's own output: bf16 in the bf16 mode with the matrix-core stem, else fp32
            get = self._act_to_host if self.stem_dtype() == B.MI_DTYPE_BF16 else self._to_host
            return get(a.init_conv_applied, N * f * Hs * Hs).reshape(N, f, Hs, Hs)
        if name == "init_conv_activated":
            return self._act_to_host(a.init_conv_activated, N * f * Hs * Hs).reshape(N, f, Hs, Hs)
        if name == "init_convblock_input":
            return self._act_to_host(a.init_convblock_input, N * f * Hp * Hp).reshape(N, f, Hp, Hp)
        if name == "max_inds":
            return self._to_host(a.max_inds, N * f * Hp * Hp, np.int32).reshape(N, f, Hp, Hp)
        if name == "final_avg_pool":
            return self._to_host(a.final_conv_output_pooled, N * d["final_depth"]).reshape(N, -1)
        if name == "fc_output":
            if deriv:
                return self._to_host(t.backprop_buffer.contents.output_layer_deriv, N * d["output"]).reshape(N, -1)
            return self._to_host(a.linear_output, N * d["output"]).reshape(N, -1)
        if name == "softmax":
            return self._to_host(t.forward_buffer.contents.pred, N * d["output"]).reshape(N, -1)
        if name.startswith("conv_blocks/"):
            _, idx, leaf = name.split("/")
            k = a.activation_conv_blocks[int(idx)].contents
            H, Ho, R, X = k.incoming_spatial_dim, k.incoming_spatial_dim // k.stride, k.reduced_depth, k.expanded_depth
            table = {"reduction_applied": ("post_reduced", R, H), "reduction_activated": ("post_reduced_activated", R, H),
                     "spatial_applied": ("post_spatial", R, Ho), "spatial_activated": ("post_spatial_activated", R, Ho),
                     "expanded_applied": ("post_expanded", X, Ho), "expanded_post_norm": ("post_expanded_norm_vals", X, Ho),
                     "transformed_residual": ("transformed_residual", X, Ho),
                     "post_projection_norm_vals": ("post_projection_norm_vals", X, Ho),
                     "combined_output": ("output", X, Ho), "output_activated": ("output_activated", X, Ho)}
            field, ch, hh = table[leaf]
            ptr = getattr(k, field)
            if not ptr:
                raise KeyError(name + " is not stored (fast path); enable full-store")
            return self._act_to_host(ptr, N * ch * hh * hh).reshape(N, ch, hh, hh)
        if name.startswith("batch_norms/"):
            parts = name.split("/")
            if parts[1] == "init":
                cache = a.norm_init_conv.contents
            else:
                k = a.activation_conv_blocks[int(parts[1])].contents
                cache = {"reduced": k.norm_post_reduced, "spatial": k.norm_post_spatial,
                         "expanded": k.norm_post_expanded, "projected": k.norm_post_projection}[parts[2]].contents
            return self._to_host(getattr(cache, parts[-1]), cache.feature_size)
        raise KeyError(name)
