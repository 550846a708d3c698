#!/usr/bin/env python3
"""Times gradient accumulation (mi_trainer_set_accumulation, include/resnet_mi.h) on the ResNet-50 arena.

kernels   the three modes of grad_accum_kernel through the operator layer on two device arrays of the arena's size, each launch
          bracketed by HIP events on its stream (mi_prof_*): FIRST moves 8 bytes per element (g in, acc out), ADD and FOLD 12
          (acc and g in, one out)
step      the ResNet-50 training step at batch 256, bf16 and fp32, momentum SGD, with k = 1 (off), 4 and 16: wall clock over --steps
          micro-batches behind --warmup (both rounded up to whole windows), the device drained at both ends; per micro-batch, and per
          applied update (k micro-batches)
  python tools/bench_accum.py [--steps 64] [--warmup 16] [--batch 256] [--only kernels|step] [--ks 1,4,16]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnet_amd import Trainer  # noqa: E402
from resnet_amd import binding as B  # noqa: E402
from resnet_amd.ops import Ops  # noqa: E402
from resnet_amd.trainer import resnet_dims  # noqa: E402

FAM_OTHER = 4


def kernels(ops, n, reps):
    L = ops.L
    rng = np.random.RandomState(0)
    acc, g = ops.dev((1e-3 * rng.randn(n)).astype(np.float32)), ops.dev((1e-3 * rng.randn(n)).astype(np.float32))
    out = {}
    for name, mode, bytes_per in (("first", B.MI_ACC_FIRST, 8.0), ("add", B.MI_ACC_ADD, 12.0), ("fold", B.MI_ACC_FOLD, 12.0)):
        def call():
            return L.mi_op_grad_accumulate(acc.ptr, g.ptr, n, mode, 0.5)
        for _ in range(3):
            assert call() == 0, L.mi_last_error()
        L.mi_prof_enable(1 << FAM_OTHER)
        L.mi_prof_reset()
        for _ in range(reps):
            assert call() == 0, L.mi_last_error()
        launches, ms, by = C.c_long(0), C.c_double(0), C.c_double(0)
        L.mi_prof_get(FAM_OTHER, C.byref(launches), C.byref(ms), None, C.byref(by))
        L.mi_prof_enable(0)
        assert launches.value == reps and by.value == bytes_per * n * reps
        per = ms.value / reps
        out[name] = dict(ms=round(per, 4), gb_per_s=round(bytes_per * n / (per * 1e-3) / 1e9, 1), bytes_per_element=int(bytes_per))
        print("%-6s %8.4f ms  %7.1f GB/s  (%d bytes per element, %.1f MB arena)" % (name, per, out[name]["gb_per_s"], bytes_per, 4.0 * n / 1e6))
    acc.free(); g.free()
    return out


def step_ms(dtype, batch, k, steps, warmup):
    """ms per micro-batch"""
    steps, warmup = -(-steps // k) * k, -(-warmup // k) * k
    tr = Trainer(resnet_dims(), batch, lr=0.01, wd=5e-5, device=0)
    try:
        tr.set_dtype(dtype)
        tr.set_optimizer("sgd")
        tr.set_loss(smoothing=0.1, device=True, copy_pred=False)
        tr.source_synthetic()
        if k > 1:
            tr.set_accumulation(k, 1.0 / k)
        for _ in range(warmup):
            tr.step()
        tr.L.mi_device_synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.load_new_batch(); tr.forward(); tr.backward(); tr.update()
        tr.L.mi_device_synchronize()
        dt = (time.perf_counter() - t0) * 1e3 / steps
        assert tr.check_errors() == 0 and tr.accumulation() == (k, 0)
        return dt
    finally:
        tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--only", choices=["kernels", "step"], default=None)
    args = ap.parse_args()
    ops = Ops()
    if ops.L.mi_device_count() < 1:
        raise RuntimeError("bench_accum needs a HIP device")
    dims = resnet_dims()
    c_flags = (C.c_int * dims["n_conv_blocks"])(*dims["is_block_spatial_reduction"])
    c_dims = ops.L.init_dimensions(dims["input"], 7, dims["init_conv_filters"], 2, 3, 2, dims["n_conv_blocks"], c_flags, dims["final_depth"], dims["output"])
    arena = int(ops.L.mi_debug_arena_floats(c_dims))
    out = {"arena_floats": arena}
    if args.only in (None, "kernels"):
        out["kernels"] = kernels(ops, arena, 50)
    if args.only in (None, "step"):
        ks = [int(k) for k in args.ks.split(",")]
        out["step_ms"] = {}
        for name in args.dtypes.split(","):
            dt = {"bf16": B.MI_DTYPE_BF16, "fp32": B.MI_DTYPE_F32}[name]
            row = {}
            for k in ks:
                per = step_ms(dt, args.batch, k, args.steps, args.warmup)
                row["k%d" % k] = dict(micro_batch_ms=round(per, 3), update_ms=round(per * k, 3))
                print("step %s batch %d, k = %2d: %.3f ms per micro-batch, %.3f ms per applied update (%d images)" % (name, args.batch, k, per, per * k, k * args.batch))
            out["step_ms"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
