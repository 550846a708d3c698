"""numpy-in / numpy-out access to the operator layer of the C-ABI (mi_op_*, include/resnet_mi.h):
device buffers are allocated, filled, the HIP kernel runs, results are copied back.  Arrays are NCHW
float32 (weights KCRS).  Used by the parity tests; the trainer calls the same kernels stream-ordered."""
import ctypes as C

import numpy as np

from . import binding as B


class DeviceArray:
    def __init__(self, lib, arr=None, shape=None, dtype=np.float32):
        self.L = lib
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            shape, dtype = arr.shape, arr.dtype
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = lib.mi_malloc(max(self.nbytes, 4))
        if not self.ptr:
            raise MemoryError(lib.mi_last_error().decode())
        if arr is not None:
            lib.mi_copy_to_device(self.ptr, arr.ctypes.data, self.nbytes)

    def get(self):
        out = np.empty(self.shape, self.dtype)
        self.L.mi_copy_to_host(out.ctypes.data, self.ptr, self.nbytes)
        return out

    def free(self):
        if self.ptr:
            self.L.mi_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def layer_routes(lib, dtype, policy, N, Cc, H, K, k, stride, site=0):
    """mi_layer_routes (host only): the planner's (fwd, dgrad, wgrad, fz) for one convolution under the process's switches, or None
    where it refuses (-2)"""
    out = (C.c_int * 4)()
    rc = lib.mi_layer_routes(dtype, policy, N, Cc, H, K, k, stride, site, out)
    return tuple(out) if rc == 0 else None

def layer_kernels(lib, dtype, policy, N, Cc, H, K, k, stride, site=0):
    """mi_layer_kernels (host only): the kernel ids (binding.MI_K_*) of the forward, the dgrad and the weight gradient inside the routes
    layer_routes answers, or None where the planner refuses (-2)"""
    out = (C.c_int * 3)()
    rc = lib.mi_layer_kernels(dtype, policy, N, Cc, H, K, k, stride, site, out)
    return tuple(out) if rc == 0 else None


class Ops:
    def __init__(self):
        self.L = B.load()

    def dev(self, arr=None, shape=None, dtype=np.float32):
        return DeviceArray(self.L, arr, shape, dtype)

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.L.mi_last_error().decode()))

    def conv_fwd(self, x, w, stride):
        N, Cc, H, _ = x.shape
        K, _, k, _ = w.shape
        dx, dw = self.dev(x), self.dev(w)
        dy = self.dev(shape=(N, K, H // stride, H // stride))
        self._chk(self.L.mi_op_conv_fwd(dx.ptr, dw.ptr, dy.ptr, N, Cc, H, K, k, stride), "conv_fwd")
        return dy.get()

    def conv_dgrad(self, w, dy, H, stride, dx_init=None):
        K, Cc, k, _ = w.shape
        N = dy.shape[0]
        dw_, ddy = self.dev(w), self.dev(dy)
        ddx = self.dev(dx_init) if dx_init is not None else self.dev(shape=(N, Cc, H, H))
        self._chk(self.L.mi_op_conv_dgrad(dw_.ptr, ddy.ptr, ddx.ptr, N, Cc, H, K, k, stride, 0 if dx_init is None else 1), "conv_dgrad")
        return ddx.get()

    def conv_wgrad(self, x, dy, k, stride):
        N, Cc, H, _ = x.shape
        K = dy.shape[1]
        dx, ddy = self.dev(x), self.dev(dy)
        dw = self.dev(shape=(K, Cc, k, k))
        self._chk(self.L.mi_op_conv_wgrad(dx.ptr, ddy.ptr, dw.ptr, N, Cc, H, K, k, stride), "conv_wgrad")
        return dw.get()

    def bn_fwd(self, x, gamma, beta, eps, relu, residual=None):
        N, Cc, H, _ = x.shape
        dx, dg, db = self.dev(x), self.dev(gamma), self.dev(beta)
        dm, dv, dy = self.dev(shape=(Cc,)), self.dev(shape=(Cc,)), self.dev(shape=x.shape)
        if residual is None:
            self._chk(self.L.mi_op_bn_fwd(dx.ptr, dg.ptr, db.ptr, dm.ptr, dv.ptr, dy.ptr, N, Cc, H, eps, int(relu)), "bn_fwd")
        else:
            dr = self.dev(residual)
            self._chk(self.L.mi_op_bn_fwd_add_relu(dx.ptr, dg.ptr, db.ptr, dr.ptr, dm.ptr, dv.ptr, dy.ptr, N, Cc, H, eps), "bn_fwd_add_relu")
        return dm.get(), dv.get(), dy.get()

    def bn_bwd(self, x, gamma, beta, means, vars_, dy, eps, mask_mode, mask_src=None):
        N, Cc, H, _ = x.shape
        dx, dg, db, dm, dv, ddy = (self.dev(a) for a in (x, gamma, beta, means, vars_, dy))
        dmask = self.dev(mask_src) if mask_src is not None else None
        out, ogam, obet = self.dev(shape=x.shape), self.dev(shape=(Cc,)), self.dev(shape=(Cc,))
        self._chk(self.L.mi_op_bn_bwd(dx.ptr, dg.ptr, db.ptr, dm.ptr, dv.ptr, ddy.ptr, dmask.ptr if dmask else None,
                                      out.ptr, ogam.ptr, obet.ptr, N, Cc, H, eps, mask_mode), "bn_bwd")
        return out.get(), ogam.get(), obet.get()

    def bn_bwd_gate(self, x, gamma, beta, means, vars_, dy, eps, mask_src):
        """BN backward with dy gated by mask_src > 0; also returns the gated dy (mi_op_bn_bwd_gate)"""
        N, Cc, H, _ = x.shape
        dx, dg, db, dm, dv, ddy, dmask = (self.dev(a) for a in (x, gamma, beta, means, vars_, dy, mask_src))
        out, gated, ogam, obet = self.dev(shape=x.shape), self.dev(shape=x.shape), self.dev(shape=(Cc,)), self.dev(shape=(Cc,))
        self._chk(self.L.mi_op_bn_bwd_gate(dx.ptr, dg.ptr, db.ptr, dm.ptr, dv.ptr, ddy.ptr, dmask.ptr, gated.ptr, out.ptr, ogam.ptr,
                                           obet.ptr, N, Cc, H, eps), "bn_bwd_gate")
        return out.get(), ogam.get(), obet.get(), gated.get()

    def decode_u8(self, src, plan, dim_out, pad_floats=0, fill=0.0):
        """uint8 images (n, dim_in, dim_in, 3) B,G,R + int32 plan (n, 3) -> fp32 (n, 3, dim_out, dim_out) (mi_op_decode_u8).
        pad_floats > 0: the output buffer is that much longer, pre-filled with `fill`; the padding comes back as a second array"""
        src = np.ascontiguousarray(src, np.uint8)
        n, dim_in = src.shape[0], src.shape[1]
        total = n * 3 * dim_out * dim_out
        dsrc, dplan = self.dev(src), self.dev(np.ascontiguousarray(plan, np.int32))
        dout = self.dev(np.full(total + pad_floats, fill, np.float32))
        self._chk(self.L.mi_op_decode_u8(dsrc.ptr, dplan.ptr, dout.ptr, n, dim_in, dim_out), "decode_u8")
        out = dout.get()
        img = out[:total].reshape(n, 3, dim_out, dim_out)
        return (img, out[total:]) if pad_floats else img

    def resample_u8(self, src, boxes, dim_out, pad_floats=0, fill=0.0):
        """uint8 images (n, dim_in, dim_in, 3) B,G,R + int32 boxes (n, 5) (row0, col0, h, w, flip) -> fp32 (n, 3, dim_out, dim_out): every
        box resampled to dim_out x dim_out (mi_op_resample_u8).  pad_floats, fill: as decode_u8"""
        src = np.ascontiguousarray(src, np.uint8)
        n, dim_in = src.shape[0], src.shape[1]
        total = n * 3 * dim_out * dim_out
        dsrc, dbox = self.dev(src), self.dev(np.ascontiguousarray(boxes, np.int32))
        dout = self.dev(np.full(total + pad_floats, fill, np.float32))
        self._chk(self.L.mi_op_resample_u8(dsrc.ptr, dbox.ptr, dout.ptr, n, dim_in, dim_out), "resample_u8")
        out = dout.get()
        img = out[:total].reshape(n, 3, dim_out, dim_out)
        return (img, out[total:]) if pad_floats else img

    def resample_aa_u8(self, src, boxes, dim_out, virt=None, win=(0, 0), pad_floats=0, fill=0.0):
        """as resample_u8, antialiased (mi_op_resample_aa_u8): every box is scaled to virt x virt (default dim_out) as Pillow's
        Image.resize(BILINEAR) scales bytes, and the window of dim_out rows and columns at win = (row, column), or one int for both, is
        written.  pad_floats, fill: as decode_u8"""
        src = np.ascontiguousarray(src, np.uint8)
        n, dim_in = src.shape[0], src.shape[1]
        virt = dim_out if virt is None else virt
        win_row, win_col = (win, win) if np.isscalar(win) else win
        total = n * 3 * dim_out * dim_out
        dsrc, dbox = self.dev(src), self.dev(np.ascontiguousarray(boxes, np.int32))
        dout = self.dev(np.full(total + pad_floats, fill, np.float32))
        self._chk(self.L.mi_op_resample_aa_u8(dsrc.ptr, dbox.ptr, dout.ptr, n, dim_in, dim_out, int(virt), int(win_row), int(win_col)), "resample_aa_u8")
        out = dout.get()
        img = out[:total].reshape(n, 3, dim_out, dim_out)
        return (img, out[total:]) if pad_floats else img

    def maxpool_fwd(self, x, k, stride):
        N, Cc, H, _ = x.shape
        Ho = H // stride
        dx, dy, di = self.dev(x), self.dev(shape=(N, Cc, Ho, Ho)), self.dev(shape=(N, Cc, Ho, Ho), dtype=np.int32)
        self._chk(self.L.mi_op_maxpool_fwd(dx.ptr, dy.ptr, di.ptr, N, Cc, H, k, stride), "maxpool_fwd")
        return dy.get(), di.get()

    def maxpool_bwd(self, idx, dy, H, k, stride):
        N, Cc = dy.shape[:2]
        di, ddy, dx = self.dev(idx.astype(np.int32)), self.dev(dy), self.dev(shape=(N, Cc, H, H))
        self._chk(self.L.mi_op_maxpool_bwd(di.ptr, ddy.ptr, dx.ptr, N, Cc, H, k, stride), "maxpool_bwd")
        return dx.get()

    def avgpool_fwd(self, x):
        N, Cc, H, _ = x.shape
        dx, dy = self.dev(x), self.dev(shape=(N, Cc))
        self._chk(self.L.mi_op_avgpool_fwd(dx.ptr, dy.ptr, N, Cc, H), "avgpool_fwd")
        return dy.get()

    def avgpool_bwd(self, dy, H):
        N, Cc = dy.shape
        ddy, dx = self.dev(dy), self.dev(shape=(N, Cc, H, H))
        self._chk(self.L.mi_op_avgpool_bwd(ddy.ptr, dx.ptr, N, Cc, H), "avgpool_bwd")
        return dx.get()

    def relu_deriv(self, x, up):
        dx, du, do = self.dev(x), self.dev(up), self.dev(shape=x.shape)
        self._chk(self.L.mi_op_relu_deriv(dx.ptr, du.ptr, do.ptr, x.size), "relu_deriv")
        return do.get()

    def matmul(self, a, b, mode="nn"):
        da, db = self.dev(a), self.dev(b)
        if mode == "nn":
            m, k = a.shape
            n = b.shape[1]
            fn = self.L.mi_op_matmul
        elif mode == "lt":  # a is [k x m]
            k, m = a.shape
            n = b.shape[1]
            fn = self.L.mi_op_matmul_lt
        else:  # "rt": b is [n x k]
            m, k = a.shape
            n = b.shape[0]
            fn = self.L.mi_op_matmul_rt
        do = self.dev(shape=(m, n))
        self._chk(fn(da.ptr, db.ptr, do.ptr, m, k, n), "matmul_" + mode)
        return do.get()

    def softmax(self, x):
        dx, do = self.dev(x), self.dev(shape=x.shape)
        self._chk(self.L.mi_op_softmax(dx.ptr, do.ptr, x.shape[0], x.shape[1]), "softmax")
        return do.get()

    def ce_deriv(self, pred, labels):
        dp, dl, dd = self.dev(pred), self.dev(labels.astype(np.int32)), self.dev(shape=pred.shape)
        self._chk(self.L.mi_op_ce_deriv(dp.ptr, dl.ptr, dd.ptr, pred.shape[0], pred.shape[1]), "ce_deriv")
        return dd.get()

    def loss_head(self, x, labels, smoothing=0.0, topk=5, total=None):
        """mi_op_loss_head on logits x (N, L): returns (pred, dlogits, row_loss, row_rank, last, total), the two records as dicts.
        total: a DeviceArray holding a MiLossMetrics to add to (a zeroed one is made otherwise)"""
        N, L = x.shape
        dx, dl = self.dev(np.ascontiguousarray(x, np.float32)), self.dev(np.ascontiguousarray(labels, np.int32))
        dp, dd = self.dev(shape=x.shape), self.dev(shape=x.shape)
        drl, drr = self.dev(shape=(N,)), self.dev(shape=(N,), dtype=np.int32)
        nb = C.sizeof(B.MiLossMetrics)
        dlast = self.dev(np.zeros(nb, np.uint8))
        dtot = total if total is not None else self.dev(np.zeros(nb, np.uint8))
        self._chk(self.L.mi_op_loss_head(dx.ptr, dl.ptr, dp.ptr, dd.ptr, drl.ptr, drr.ptr, N, L, smoothing, topk, dlast.ptr, dtot.ptr), "loss_head")
        rec = [B.MiLossMetrics.from_buffer_copy(d.get().tobytes()).as_dict() for d in (dlast, dtot)]
        return dp.get(), dd.get(), drl.get(), drr.get(), rec[0], rec[1]

    @staticmethod
    def mix_plan_struct(mode=0, lam=1.0, box=(0, 0, 0, 0)):
        """a MiMixPlan: mode 0 none / 1 mixup / 2 CutMix, box = (y0, x0, y1, x1)"""
        return B.MiMixPlan(int(mode), float(lam), *[int(v) for v in box])

    def mix_batch(self, images, plan, offset_floats=0):
        """mi_op_mix_batch: fp32 images (n, 3, D, D) mixed in place on the device, row i with row n - 1 - i, under plan (a MiMixPlan,
        or a dict with mode, lam, y0, x0, y1, x1); returns the mixed batch.  offset_floats: the batch starts that many floats into its
        device buffer (1: a pointer that is 4- but not 16-byte aligned)"""
        images = np.ascontiguousarray(images, np.float32)
        n, _, D, _ = images.shape
        if isinstance(plan, dict):
            plan = B.MiMixPlan(plan["mode"], plan["lam"], plan["y0"], plan["x0"], plan["y1"], plan["x1"])
        buf = np.zeros(offset_floats + images.size, np.float32)
        buf[offset_floats:] = images.ravel()
        d = self.dev(buf)
        self._chk(self.L.mi_op_mix_batch(d.ptr + 4 * offset_floats, n, 3 * D * D, D, C.byref(plan)), "mix_batch")
        return d.get()[offset_floats:].reshape(images.shape)

    def mix_geometry(self):
        """(threads, cap on grid.x, waves of a workgroup) of the two mix kernels: one sweep is threads * cap work items (mixup), cap * waves
        row segments (CutMix)"""
        out = (C.c_size_t * 3)()
        self.L.mi_debug_mix_geometry(out)
        return tuple(int(v) for v in out)

    def erase_batch(self, images, boxes, mode="const", value=(0, 0, 0), std=(1, 1, 1), noise_seed=0, first_row=0, offset_floats=0):
        """mi_op_erase_batch: fp32 images (n, 3, D, D) erased in place on the device, row i inside boxes[i] = (y0, x0, h, w); mode "const"
        fills plane c with value[c], "noise" with value[c] + std[c] z (z from noise_seed, first_row + i and the element's position); returns
        the erased batch.  offset_floats: as mix_batch"""
        images = np.ascontiguousarray(images, np.float32)
        n, _, D, _ = images.shape
        boxes = np.ascontiguousarray(boxes, np.int32).reshape(n, 4)
        fill = B.erase_fill_struct(mode, value, std, noise_seed)
        buf = np.zeros(offset_floats + images.size, np.float32)
        buf[offset_floats:] = images.ravel()
        d = self.dev(buf)
        self._chk(self.L.mi_op_erase_batch(d.ptr + 4 * offset_floats, n, 3 * D * D, D, boxes.ctypes.data, C.byref(fill), int(first_row)), "erase_batch")
        return d.get()[offset_floats:].reshape(images.shape)

    def erase_geometry(self):
        """(threads, cap on grid.x, waves of a workgroup, rows of a launch) of erase_kernel: one sweep of the capped grid is cap * waves row
        segments of a row's box; a batch of more rows than a launch carries takes several launches"""
        out = (C.c_size_t * 4)()
        self.L.mi_debug_erase_geometry(out)
        return tuple(int(v) for v in out)

    def ta_row(self, op, bin, neg, dim):
        """mi_ta_row: the record of one operation, strength bin and sign on a dim x dim image, as a dict"""
        r = B.MiTaRow()
        self._chk(self.L.mi_ta_row(int(op), int(bin), int(neg), int(dim), C.byref(r)), "ta_row")
        return r.as_dict()

    def ta_plan(self, seed, epoch, step, rank, world, n, dim):
        """mi_ta_plan: the records of one step's n rows, a list of dicts"""
        rows = (B.MiTaRow * max(n, 1))()
        self._chk(self.L.mi_ta_plan(int(seed) & (2 ** 64 - 1), int(epoch), int(step), int(rank), int(world), int(n), int(dim), rows), "ta_plan")
        return [rows[i].as_dict() for i in range(n)]

    def trivial_augment(self, images, rows, offset_floats=0, workspace=None, keep_workspace=False, n=None):
        """mi_op_trivial_augment: fp32 images (n, 3, D, D) augmented in place on the device, row i under rows[i] (dicts as ta_row gives
        them); returns the augmented batch.  offset_floats: as mix_batch.  workspace: a device buffer of an earlier call to run over again
        (keep_workspace=True returns (batch, workspace)).  n: only the first n rows belong to the call, the rest of the buffer lies behind it"""
        images = np.ascontiguousarray(images, np.float32)
        D = images.shape[2]
        n = images.shape[0] if n is None else int(n)
        arr = B.ta_rows_struct(rows)
        buf = np.zeros(offset_floats + images.size, np.float32)
        buf[offset_floats:] = images.ravel()
        d = self.dev(buf)
        if workspace is None:
            workspace = self.dev(np.full(int(self.L.mi_ta_workspace_bytes(n, D)), 0xA5, np.uint8))  # arbitrary contents
        self._chk(self.L.mi_op_trivial_augment(d.ptr + 4 * offset_floats, n, 3 * D * D, D, arr, workspace.ptr), "trivial_augment")
        out = d.get()[offset_floats:].reshape(images.shape)
        return (out, workspace) if keep_workspace else out

    def ta_geometry(self):
        """(threads, cap on grid.x, rows of a launch, pixels a thread takes per turn on the 16-byte path) of the two kernels"""
        out = (C.c_size_t * 4)()
        self.L.mi_debug_ta_geometry(out)
        return tuple(int(v) for v in out)

    def loss_head_mix(self, x, labels_a, labels_b, lam, smoothing=0.0, topk=5, total=None):
        """mi_op_loss_head_mix on logits x (N, L) with two labels per row and the weight lam: returns what loss_head returns"""
        N, L = x.shape
        dx = self.dev(np.ascontiguousarray(x, np.float32))
        da, db = self.dev(np.ascontiguousarray(labels_a, np.int32)), self.dev(np.ascontiguousarray(labels_b, np.int32))
        dp, dd = self.dev(shape=x.shape), self.dev(shape=x.shape)
        drl, drr = self.dev(shape=(N,)), self.dev(shape=(N,), dtype=np.int32)
        nb = C.sizeof(B.MiLossMetrics)
        dlast = self.dev(np.zeros(nb, np.uint8))
        dtot = total if total is not None else self.dev(np.zeros(nb, np.uint8))
        self._chk(self.L.mi_op_loss_head_mix(dx.ptr, da.ptr, db.ptr, float(lam), dp.ptr, dd.ptr, drl.ptr, drr.ptr, N, L, smoothing, topk, dlast.ptr,
                                             dtot.ptr), "loss_head_mix")
        rec = [B.MiLossMetrics.from_buffer_copy(d.get().tobytes()).as_dict() for d in (dlast, dtot)]
        return dp.get(), dd.get(), drl.get(), drr.get(), rec[0], rec[1]

    def bn_running_update(self, means, vars_, counts, running, momentum, guard=0, fill=0.0):
        """mi_op_bn_running_update: lists of per-layer batch means / biased vars (float32, [C_i] each) and sample counts, running (2, R)
        float32 with R >= sum C_i (layer i at the sum of the channels before it in both rows).  Returns the updated (2, R) array;
        guard > 0: that many floats of `fill` lie in front of and behind the arena in the same allocation and come back as well"""
        running = np.ascontiguousarray(running, np.float32)
        R = running.shape[1]
        pad = np.full(guard, fill, np.float32)
        buf = self.dev(np.concatenate([pad, running.ravel(), pad]))
        dm = [self.dev(np.ascontiguousarray(a, np.float32)) for a in means]
        dv = [self.dev(np.ascontiguousarray(a, np.float32)) for a in vars_]
        n = len(dm)
        pm, pv = (C.c_void_p * n)(*[d.ptr for d in dm]), (C.c_void_p * n)(*[d.ptr for d in dv])
        ch = (C.c_int * n)(*[int(np.size(a)) for a in means])
        cnt = (C.c_int64 * n)(*[int(c) for c in counts])
        self._chk(self.L.mi_op_bn_running_update(pm, pv, ch, cnt, n, buf.ptr + 4 * guard, R, momentum), "bn_running_update")
        out = buf.get()
        new = out[guard:guard + 2 * R].reshape(2, R)
        return (new, out[:guard], out[guard + 2 * R:]) if guard else new

    def _guarded(self, arr, offset_floats, guard, fill):
        """arr (float32 or uint32 words) in an allocation of its own: offset_floats + guard words of `fill` in front of it, guard behind.
        Returns (device array, word offset of arr, host dtype)"""
        arr = np.ascontiguousarray(arr).ravel()
        assert arr.dtype.itemsize == 4
        pad = np.full(guard, fill, np.float32).view(arr.dtype)
        lead = np.full(offset_floats, fill, np.float32).view(arr.dtype)
        return self.dev(np.concatenate([lead, pad, arr, pad])), offset_floats + guard

    def ema_geometry(self):
        """(threads, floats of one workgroup's turn in the vector / the element-wise instantiation, grid cap) of the two kernels below"""
        out = (C.c_size_t * 4)()
        self.L.mi_debug_ema_geometry(out)
        return tuple(int(v) for v in out)

    def ema_update(self, ema, p, w, offset_floats=0, guard=0, fill=0.0):
        """mi_op_ema_update: ema <- lerp(ema, p, w) on float32 arrays of one length.  Both operands start offset_floats floats (+ the guard)
        into 16-byte-aligned allocations of their own (0 with a guard that is a multiple of 4: the vector instantiation, 1: the element-wise
        one).  Returns (ema, p); guard > 0: each as (values, guard in front, guard behind), the guards pre-filled with `fill`"""
        n = int(np.size(ema))
        de, at = self._guarded(np.asarray(ema, np.float32), offset_floats, guard, fill)
        dp, _ = self._guarded(np.asarray(p, np.float32), offset_floats, guard, fill)
        self._chk(self.L.mi_op_ema_update(de.ptr + 4 * at, dp.ptr + 4 * at, n, float(w)), "ema_update")
        return self._unguard(de, at, n, guard), self._unguard(dp, at, n, guard)

    def exchange(self, a, b, offset_floats=0, guard=0, fill=0.0):
        """mi_op_exchange: a <-> b as 32-bit words (float32 or uint32 arrays of one length); operands placed and returned as ema_update's"""
        n = int(np.size(a))
        da, at = self._guarded(a, offset_floats, guard, fill)
        db, _ = self._guarded(b, offset_floats, guard, fill)
        self._chk(self.L.mi_op_exchange(da.ptr + 4 * at, db.ptr + 4 * at, n), "exchange")
        return self._unguard(da, at, n, guard), self._unguard(db, at, n, guard)

    def accum_geometry(self):
        """(threads, floats of one workgroup's turn in the vector / the element-wise instantiation, grid cap) of grad_accumulate's kernel"""
        out = (C.c_size_t * 4)()
        self.L.mi_debug_accum_geometry(out)
        return tuple(int(v) for v in out)

    def grad_accumulate(self, acc, g, mode, scale=1.0, offset_floats=0, guard=0, fill=0.0):
        """mi_op_grad_accumulate on float32 (or uint32) arrays of one length: mode MI_ACC_FIRST acc = g, MI_ACC_ADD acc = acc + g, MI_ACC_FOLD
        g = (acc + g) * scale.  Operands placed and returned as ema_update's: (acc, g)"""
        n = int(np.size(acc))
        da, at = self._guarded(acc, offset_floats, guard, fill)
        dg, _ = self._guarded(g, offset_floats, guard, fill)
        self._chk(self.L.mi_op_grad_accumulate(da.ptr + 4 * at, dg.ptr + 4 * at, n, int(mode), float(scale)), "grad_accumulate")
        return self._unguard(da, at, n, guard), self._unguard(dg, at, n, guard)

    @staticmethod
    def _unguard(d, at, n, guard):
        out = d.get()
        return (out[at:at + n], out[at - guard:at], out[at + n:]) if guard else out[at:at + n]

    def adam(self, p, g, m, v, lr, wd, b1, b2, cur_b1, cur_b2, eps):
        dp, dg, dm, dv = (self.dev(a) for a in (p, g, m, v))
        flag = self.dev(np.zeros(1, np.int32))
        self._chk(self.L.mi_op_adam(dp.ptr, dg.ptr, dm.ptr, dv.ptr, p.size, lr, wd, b1, b2, cur_b1, cur_b2, eps, flag.ptr), "adam")
        return dp.get(), dm.get(), dv.get(), int(flag.get()[0])

    def clip_grad_norm(self, g, offsets, max_norm):
        """mi_op_clip_grad_norm on a float32 array: tensor i = [offsets[i], offsets[i + 1]).  Returns (g, the record as a dict)"""
        dg = self.dev(np.ascontiguousarray(g, np.float32).ravel())
        off = np.ascontiguousarray(offsets, np.uint64)
        r = B.MiClipRecord()
        self._chk(self.L.mi_op_clip_grad_norm(dg.ptr, int(np.size(g)), off.ctypes.data, len(off) - 1, float(max_norm), C.byref(r)), "clip_grad_norm")
        return dg.get(), r.as_dict()

    def momentum_update(self, kind, p, g, b, offsets, is_weight, lr, wd, momentum, trust=0.001, wd_norm=None):
        """mi_op_momentum_update over one arena: p, g, b float32 arrays of the same length, tensor i = [offsets[i], offsets[i + 1]).
        wd_norm (SGD): the decay of the tensors with is_weight 0, None: wd (mi_op_momentum_update2).
        Returns (p, g, b, NaN flag, squared norms [n_tensors, 2] as (|w|^2, |g|^2) before the update)"""
        dp, dg, db = (self.dev(np.ascontiguousarray(a, np.float32)) for a in (p, g, b))
        flag = self.dev(np.zeros(1, np.int32))
        off = np.ascontiguousarray(offsets, np.uint64)
        isw = np.ascontiguousarray(is_weight, np.int32)
        n_t = len(off) - 1
        assert isw.size == n_t and C.sizeof(C.c_size_t) == 8
        sq = np.zeros((n_t, 2), np.float64)
        if wd_norm is None:
            self._chk(self.L.mi_op_momentum_update(int(kind), dp.ptr, dg.ptr, db.ptr, p.size, off.ctypes.data, n_t, isw.ctypes.data, lr, wd,
                                                   momentum, trust, flag.ptr, sq.ctypes.data), "momentum_update")
        else:
            self._chk(self.L.mi_op_momentum_update2(int(kind), dp.ptr, dg.ptr, db.ptr, p.size, off.ctypes.data, n_t, isw.ctypes.data, lr, wd,
                                                    float(wd_norm), momentum, trust, flag.ptr, sq.ctypes.data), "momentum_update2")
        return dp.get(), dg.get(), db.get(), int(flag.get()[0]), sq

    def nhwc_to_nchw(self, x):
        N, H, W, Cc = x.shape
        dx, do = self.dev(x), self.dev(shape=(N, Cc, H, W))
        self._chk(self.L.mi_op_nhwc_to_nchw(dx.ptr, do.ptr, N, H, W, Cc), "nhwc_to_nchw")
        return do.get()

    # ---- typed operators: activation tensors stored as bf16 on the device, numpy float32 at this boundary ----
    # (values are rounded to bf16 -- round to nearest even -- on the way in; outputs come back widened, so a bf16 result
    # is a float32 array whose values are exactly the stored bf16 numbers)
    def dev_t(self, arr, dt):
        """upload a float32 array as a tensor of storage type dt"""
        d32 = self.dev(np.ascontiguousarray(arr, np.float32))
        if dt == B.MI_DTYPE_F32:
            return d32
        out = DeviceArray(self.L, shape=arr.shape, dtype=np.uint16)
        self._chk(self.L.mi_op_convert(d32.ptr, B.MI_DTYPE_F32, out.ptr, B.MI_DTYPE_BF16, arr.size), "convert")
        return out

    def new_t(self, shape, dt):
        return DeviceArray(self.L, shape=shape, dtype=np.float32 if dt == B.MI_DTYPE_F32 else np.uint16)

    def get_t(self, darr, dt):
        if dt == B.MI_DTYPE_F32:
            return darr.get()
        out = self.dev(shape=darr.shape)
        self._chk(self.L.mi_op_convert(darr.ptr, B.MI_DTYPE_BF16, out.ptr, B.MI_DTYPE_F32, int(np.prod(darr.shape))), "convert")
        return out.get()

    def conv_fwd_bf16(self, x, w, stride):
        N, Cc, H, _ = x.shape
        K, _, k, _ = w.shape
        BF = B.MI_DTYPE_BF16
        dx, dw = self.dev_t(x, BF), self.dev(w)
        dy = self.new_t((N, K, H // stride, H // stride), BF)
        self._chk(self.L.mi_op_conv_fwd_bf16(dx.ptr, dw.ptr, dy.ptr, N, Cc, H, K, k, stride), "conv_fwd_bf16")
        return self.get_t(dy, BF)

    def conv_fwd_bf16_cl(self, x, w, stride):
        """3x3 forward on channel-last zero-padded operands (kernels_cl_bf16.hip)"""
        N, Cc, H, _ = x.shape
        K = w.shape[0]
        BF = B.MI_DTYPE_BF16
        dx, dw = self.dev_t(x, BF), self.dev(w)
        dy = self.new_t((N, K, H // stride, H // stride), BF)
        self._chk(self.L.mi_op_conv_fwd_bf16_cl(dx.ptr, dw.ptr, dy.ptr, N, Cc, H, K, stride), "conv_fwd_bf16_cl")
        return self.get_t(dy, BF)

    def conv_wgrad_bf16_cl(self, x, dy, stride):
        N, Cc, H, _ = x.shape
        K = dy.shape[1]
        BF = B.MI_DTYPE_BF16
        dx, ddy = self.dev_t(x, BF), self.dev_t(dy, BF)
        dw = self.dev(shape=(K, Cc, 3, 3))
        self._chk(self.L.mi_op_conv_wgrad_bf16_cl(dx.ptr, ddy.ptr, dw.ptr, N, Cc, H, K, stride), "conv_wgrad_bf16_cl")
        return dw.get()

    def bn_fwd_cl_bf16(self, x, gamma, beta, eps, residual=None, par=False):
        """BN (+ residual) + ReLU written twice (bn_apply_cl_kernel): returns means, vars, y (NCHW) and the channel-last copy -- one plane
        [N][H+2][H+2][C], or (par) the four parity planes [N][4][H/2+1][H/2+1][C]"""
        N, Cc, H, _ = x.shape
        BF = B.MI_DTYPE_BF16
        dx, dg, db = self.dev_t(x, BF), self.dev(gamma), self.dev(beta)
        dr = self.dev_t(residual, BF) if residual is not None else None
        dm, dv, dy = self.dev(shape=(Cc,)), self.dev(shape=(Cc,)), self.new_t(x.shape, BF)
        shp = (N, 4, H // 2 + 1, H // 2 + 1, Cc) if par else (N, H + 2, H + 2, Cc)
        ycl = self.dev_t(np.zeros(shp, np.float32), BF)   # zero halo
        self._chk(self.L.mi_op_bn_fwd_cl_bf16(dx.ptr, dg.ptr, db.ptr, dr.ptr if dr else None, dm.ptr, dv.ptr, dy.ptr, ycl.ptr, N, Cc, H, eps, int(par)),
                  "bn_fwd_cl_bf16")
        return dm.get(), dv.get(), self.get_t(dy, BF), self.get_t(ycl, BF)

    def conv1x1_fwd_bf16_cl(self, x, w):
        N, Cc, H, _ = x.shape
        K = w.shape[0]
        BF = B.MI_DTYPE_BF16
        dx, dw = self.dev_t(x, BF), self.dev(w)
        dy = self.new_t((N, K, H, H), BF)
        self._chk(self.L.mi_op_conv1x1_fwd_bf16_cl(dx.ptr, dw.ptr, dy.ptr, N, Cc, H, K), "conv1x1_fwd_bf16_cl")
        return self.get_t(dy, BF)

    def conv_wgrad_bf16_cl2(self, x, dy, stride=2):
        """3x3, both operands re-laid channel-last (cl_wgrad2_kernel)"""
        N, Cc, H, _ = x.shape
        K = dy.shape[1]
        BF = B.MI_DTYPE_BF16
        dx, ddy = self.dev_t(x, BF), self.dev_t(dy, BF)
        dw = self.dev(shape=(K, Cc, 3, 3))
        self._chk(self.L.mi_op_conv_wgrad_bf16_cl2(dx.ptr, ddy.ptr, dw.ptr, N, Cc, H, K, stride), "conv_wgrad_bf16_cl2")
        return dw.get()

    def conv_dgrad_bf16_cl(self, w, dy, H, dx_init=None, stride=1):
        K, Cc, k, _ = w.shape
        N = dy.shape[0]
        BF = B.MI_DTYPE_BF16
        dw_, ddy = self.dev(w), self.dev_t(dy, BF)
        ddx = self.dev_t(dx_init, BF) if dx_init is not None else self.new_t((N, Cc, H, H), BF)
        self._chk(self.L.mi_op_conv_dgrad_bf16_cl(dw_.ptr, ddy.ptr, ddx.ptr, N, Cc, H, K, stride, 0 if dx_init is None else 1), "conv_dgrad_bf16_cl")
        return self.get_t(ddx, BF)

    def conv_dgrad_bf16(self, w, dy, H, stride, dx_init=None):
        K, Cc, k, _ = w.shape
        N = dy.shape[0]
        BF = B.MI_DTYPE_BF16
        dw_, ddy = self.dev(w), self.dev_t(dy, BF)
        ddx = self.dev_t(dx_init, BF) if dx_init is not None else self.new_t((N, Cc, H, H), BF)
        self._chk(self.L.mi_op_conv_dgrad_bf16(dw_.ptr, ddy.ptr, ddx.ptr, N, Cc, H, K, k, stride, 0 if dx_init is None else 1), "conv_dgrad_bf16")
        return self.get_t(ddx, BF)

    def conv_wgrad_bf16(self, x, dy, k, stride):
        N, Cc, H, _ = x.shape
        K = dy.shape[1]
        BF = B.MI_DTYPE_BF16
        dx, ddy = self.dev_t(x, BF), self.dev_t(dy, BF)
        dw = self.dev(shape=(K, Cc, k, k))
        self._chk(self.L.mi_op_conv_wgrad_bf16(dx.ptr, ddy.ptr, dw.ptr, N, Cc, H, K, k, stride), "conv_wgrad_bf16")
        return dw.get()

    def bn_fwd_t(self, x, gamma, beta, eps, relu, x_dt, a_dt, residual=None):
        N, Cc, H, _ = x.shape
        dx, dg, db = self.dev_t(x, x_dt), self.dev(gamma), self.dev(beta)
        dm, dv, dy = self.dev(shape=(Cc,)), self.dev(shape=(Cc,)), self.new_t(x.shape, a_dt)
        dr = self.dev_t(residual, a_dt) if residual is not None else None
        self._chk(self.L.mi_op_bn_fwd_t(dx.ptr, x_dt, dg.ptr, db.ptr, dr.ptr if dr else None, dm.ptr, dv.ptr, dy.ptr, a_dt, N, Cc, H, eps,
                                        int(relu)), "bn_fwd_t")
        return dm.get(), dv.get(), self.get_t(dy, a_dt)

    def conv_dgrad_bn_bwd_bf16(self, w, dy, H, stride, bn_x, mask, gamma, beta, means, vars_, eps, addend=None):
        """dgrad + the BN(+ReLU) backward in front of it, chained as backwards_pass does; returns gated dy, bn dx, dgamma, dbeta, fused?"""
        N = dy.shape[0]
        K, Cc, k, _ = w.shape
        BF = B.MI_DTYPE_BF16
        dw, ddy = self.dev(w), self.dev_t(dy, BF)
        dadd = self.dev_t(addend, BF) if addend is not None else None
        dxb, dmask = self.dev_t(bn_x, BF), self.dev_t(mask, BF)
        dg, db, dm, dv = (self.dev(a) for a in (gamma, beta, means, vars_))
        gated, bdx = self.new_t((N, Cc, H, H), BF), self.new_t((N, Cc, H, H), BF)
        og, ob = self.dev(shape=(Cc,)), self.dev(shape=(Cc,))
        rc = self.L.mi_op_conv_dgrad_bn_bwd_bf16(dw.ptr, ddy.ptr, dadd.ptr if dadd else None, gated.ptr, N, Cc, H, K, k, stride, dxb.ptr, dmask.ptr,
                                                 dg.ptr, db.ptr, dm.ptr, dv.ptr, eps, bdx.ptr, og.ptr, ob.ptr)
        if rc < 0:
            self._chk(rc, "conv_dgrad_bn_bwd_bf16")
        return self.get_t(gated, BF), self.get_t(bdx, BF), og.get(), ob.get(), rc > 0

    def conv_dgrad_bn_bwd_f32(self, w, dy, H, stride, bn_x, mask, gamma, beta, means, vars_, eps, addend=None):
        """fp32 twin of conv_dgrad_bn_bwd_bf16"""
        N = dy.shape[0]
        K, Cc, k, _ = w.shape
        dw, ddy = self.dev(w), self.dev(dy)
        dadd = self.dev(addend) if addend is not None else None
        dxb, dmask = self.dev(bn_x), self.dev(mask)
        dg, db, dm, dv = (self.dev(a) for a in (gamma, beta, means, vars_))
        gated, bdx = self.dev(shape=(N, Cc, H, H)), self.dev(shape=(N, Cc, H, H))
        og, ob = self.dev(shape=(Cc,)), self.dev(shape=(Cc,))
        rc = self.L.mi_op_conv_dgrad_bn_bwd_f32(dw.ptr, ddy.ptr, dadd.ptr if dadd else None, gated.ptr, N, Cc, H, K, k, stride, dxb.ptr, dmask.ptr,
                                                dg.ptr, db.ptr, dm.ptr, dv.ptr, eps, bdx.ptr, og.ptr, ob.ptr)
        if rc < 0:
            self._chk(rc, "conv_dgrad_bn_bwd_f32")
        return gated.get(), bdx.get(), og.get(), ob.get(), rc > 0

    def stem_fwd_bf16(self, x, w, exact=False):
        """the matrix-core stem: operands rounded to bf16, or (exact) fp32 arithmetic"""
        N, _, H, _ = x.shape
        dx, dw, dy = self.dev(x), self.dev(w), self.dev(shape=(N, 64, H // 2, H // 2))
        fn = self.L.mi_op_stem_fwd_f32 if exact else self.L.mi_op_stem_fwd_bf16
        self._chk(fn(dx.ptr, dw.ptr, dy.ptr, N, H), "stem_fwd")
        return dy.get()

    def stem_wgrad_bf16(self, x, w, dy, exact=False):
        N, _, H, _ = x.shape
        dx, dw, ddy, out = self.dev(x), self.dev(w), self.dev(dy), self.dev(shape=w.shape)
        fn = self.L.mi_op_stem_wgrad_f32 if exact else self.L.mi_op_stem_wgrad_bf16
        self._chk(fn(dx.ptr, dw.ptr, ddy.ptr, out.ptr, N, H), "stem_wgrad")
        return out.get()

    def conv_bn_fwd_t(self, x, w, gamma, beta, stride, eps, relu, dt):
        """conv + BN as forward_pass pairs them; returns conv_out, means, vars, y and whether the statistics were fused"""
        N, Cc, H, _ = x.shape
        K, _, k, _ = w.shape
        Ho = H // stride
        dx, dw, dg, db = self.dev_t(x, dt), self.dev(w), self.dev(gamma), self.dev(beta)
        dc, dy = self.new_t((N, K, Ho, Ho), dt), self.new_t((N, K, Ho, Ho), dt)
        dm, dv = self.dev(shape=(K,)), self.dev(shape=(K,))
        rc = self.L.mi_op_conv_bn_fwd_t(dx.ptr, dw.ptr, dc.ptr, dt, dg.ptr, db.ptr, dm.ptr, dv.ptr, dy.ptr, N, Cc, H, K, k, stride, eps, int(relu))
        if rc < 0:
            self._chk(rc, "conv_bn_fwd_t")
        return self.get_t(dc, dt), dm.get(), dv.get(), self.get_t(dy, dt), rc > 0

    def conv_bn_fwd_bf16_cl(self, x, w, gamma, beta, stride, eps, relu):
        """conv + BN on the channel-last 3x3 forward (the bf16 trainer's MI_FWD_CL); returns as conv_bn_fwd_t"""
        N, Cc, H, _ = x.shape
        K = w.shape[0]
        Ho = H // stride
        BF = B.MI_DTYPE_BF16
        dx, dw, dg, db = self.dev_t(x, BF), self.dev(w), self.dev(gamma), self.dev(beta)
        dc, dy = self.new_t((N, K, Ho, Ho), BF), self.new_t((N, K, Ho, Ho), BF)
        dm, dv = self.dev(shape=(K,)), self.dev(shape=(K,))
        rc = self.L.mi_op_conv_bn_fwd_bf16_cl(dx.ptr, dw.ptr, dc.ptr, dg.ptr, db.ptr, dm.ptr, dv.ptr, dy.ptr, N, Cc, H, K, stride, eps, int(relu))
        if rc < 0:
            self._chk(rc, "conv_bn_fwd_bf16_cl")
        return self.get_t(dc, BF), dm.get(), dv.get(), self.get_t(dy, BF), rc > 0

    def stem_bn_fwd_t(self, x, w, gamma, beta, eps, conv_dt, a_dt, exact):
        """the matrix-core stem + BN + ReLU (MI_FWD_STEM_F32 with exact, else MI_FWD_STEM_BF16); conv_out stored as conv_dt, y as a_dt;
        returns as conv_bn_fwd_t"""
        N, _, H, _ = x.shape
        Ho = H // 2
        dx, dw, dg, db = self.dev(x), self.dev(w), self.dev(gamma), self.dev(beta)
        dc, dy = self.new_t((N, 64, Ho, Ho), conv_dt), self.new_t((N, 64, Ho, Ho), a_dt)
        dm, dv = self.dev(shape=(64,)), self.dev(shape=(64,))
        rc = self.L.mi_op_stem_bn_fwd_t(dx.ptr, dw.ptr, dc.ptr, conv_dt, dg.ptr, db.ptr, dm.ptr, dv.ptr, dy.ptr, a_dt, N, H, eps, int(exact))
        if rc < 0:
            self._chk(rc, "stem_bn_fwd_t")
        return self.get_t(dc, conv_dt), dm.get(), dv.get(), self.get_t(dy, a_dt), rc > 0

    def stem_wgrad_bf16_t(self, x, w, dy, dy_dt):
        """the bf16 stem's weight gradient from dy stored as dy_dt"""
        N, _, H, _ = x.shape
        dx, dw, ddy, out = self.dev(x), self.dev(w), self.dev_t(dy, dy_dt), self.dev(shape=w.shape)
        self._chk(self.L.mi_op_stem_wgrad_bf16_t(dx.ptr, dw.ptr, ddy.ptr, dy_dt, out.ptr, N, H), "stem_wgrad_bf16_t")
        return out.get()

    def bn_apply_t(self, x, gamma, beta, means, vars_, eps, relu, x_dt, a_dt, residual=None):
        N, Cc, H, _ = x.shape
        dx, dg, db, dm, dv = self.dev_t(x, x_dt), self.dev(gamma), self.dev(beta), self.dev(means), self.dev(vars_)
        dy = self.new_t(x.shape, a_dt)
        dr = self.dev_t(residual, a_dt) if residual is not None else None
        self._chk(self.L.mi_op_bn_apply_t(dx.ptr, x_dt, dg.ptr, db.ptr, dr.ptr if dr else None, dm.ptr, dv.ptr, dy.ptr, a_dt, N, Cc, H, eps,
                                          int(relu)), "bn_apply_t")
        return self.get_t(dy, a_dt)

    def bn_bwd_t(self, x, gamma, beta, means, vars_, dy, eps, mask_mode, x_dt, a_dt, mask_src=None):
        """returns dx, dgamma, dbeta (and the gated dy for mask_mode 3)"""
        N, Cc, H, _ = x.shape
        dx, ddy = self.dev_t(x, x_dt), self.dev_t(dy, a_dt)
        dg, db, dm, dv = (self.dev(a) for a in (gamma, beta, means, vars_))
        dmask = self.dev_t(mask_src, a_dt) if mask_src is not None else None
        gated = self.new_t(x.shape, a_dt) if mask_mode == 3 else None
        out, ogam, obet = self.new_t(x.shape, x_dt), self.dev(shape=(Cc,)), self.dev(shape=(Cc,))
        self._chk(self.L.mi_op_bn_bwd_t(dx.ptr, x_dt, dg.ptr, db.ptr, dm.ptr, dv.ptr, ddy.ptr, dmask.ptr if dmask else None,
                                        gated.ptr if gated else None, a_dt, out.ptr, ogam.ptr, obet.ptr, N, Cc, H, eps, mask_mode), "bn_bwd_t")
        res = (self.get_t(out, x_dt), ogam.get(), obet.get())
        return res + (self.get_t(gated, a_dt),) if gated else res

    def maxpool_fwd_t(self, x, k, stride, dt):
        N, Cc, H, _ = x.shape
        Ho = H // stride
        dx, dy, di = self.dev_t(x, dt), self.new_t((N, Cc, Ho, Ho), dt), self.dev(shape=(N, Cc, Ho, Ho), dtype=np.int32)
        self._chk(self.L.mi_op_maxpool_fwd_t(dx.ptr, dy.ptr, dt, di.ptr, N, Cc, H, k, stride), "maxpool_fwd_t")
        return self.get_t(dy, dt), di.get()

    def maxpool_bwd_t(self, idx, dy, H, k, stride, dt):
        N, Cc = dy.shape[:2]
        di, ddy, dx = self.dev(idx.astype(np.int32)), self.dev_t(dy, dt), self.new_t((N, Cc, H, H), dt)
        self._chk(self.L.mi_op_maxpool_bwd_t(di.ptr, ddy.ptr, dx.ptr, dt, N, Cc, H, k, stride), "maxpool_bwd_t")
        return self.get_t(dx, dt)

    def avgpool_fwd_t(self, x, dt):
        N, Cc, H, _ = x.shape
        dx, dy = self.dev_t(x, dt), self.dev(shape=(N, Cc))
        self._chk(self.L.mi_op_avgpool_fwd_t(dx.ptr, dt, dy.ptr, N, Cc, H), "avgpool_fwd_t")
        return dy.get()

    def avgpool_bwd_t(self, dy, H, dt):
        N, Cc = dy.shape
        ddy, dx = self.dev(dy), self.new_t((N, Cc, H, H), dt)
        self._chk(self.L.mi_op_avgpool_bwd_t(ddy.ptr, dx.ptr, dt, N, Cc, H), "avgpool_bwd_t")
        return self.get_t(dx, dt)
