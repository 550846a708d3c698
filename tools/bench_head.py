#!/usr/bin/env python3
"""What the classification head costs, on the host path and on the device (mi_trainer_set_loss, include/resnet_mi.h).

  head   N = 256, L = 1000, on the logits of a real forward pass (a one-block network at batch 256), ms per call, host clock around calls
         that end in a stream synchronise:
           (a) the head as forward_pass / backwards_pass run it by default, call for call: soft-max, the copy of pred to pinned host
               memory, stream synchronise, mi_host_loss, the cross-entropy derivative (+ a synchronise so that its run time counts)
           (b) mi_op_loss_head (head + reduce launch, one synchronise), and (b) followed by the 40-byte copy of the record to the host
         The legs alternate in five rounds of head-calls / 5 calls each; median, minimum and 90th percentile over all calls.
         (a) calls the library's stream-ordered launchers (mid_*: exported, not part of include/resnet_mi.h) so that it synchronises
         where the trainer does, not after every launch as the mi_op_* operators do.
  step   ResNet-50 at batch 256 from the synthetic source, one process per storage type, ONE trainer whose head is switched between
         blocks of steps (the setting may change between steps), the modes alternating block by block so that drift hits all alike:
           host          MI_LOSS_HOST, the reference's main loop (load, forward, mi_host_loss, backward, update)
           device        MI_LOSS_DEVICE | MI_LOSS_NO_PRED_COPY, the same loop: mi_host_loss reads the device's record every step
           device_async  the same flags without the per-step loss: the totals are read once per block (mi_trainer_metrics)
         ms per step = block time / steps, host clock from a device synchronise to a device synchronise; per mode the median over the
         blocks and the spread (max - min) of its blocks.
A library without mi_trainer_set_loss (an older build through RESNET_MI_LIB, or this file copied into an older tree) runs the host legs only.

  python tools/bench_head.py [--steps 10] [--blocks 5] [--warmup 5] [--batch 256] [--head-calls 200] [--skip-head] [--dtypes f32,bf16]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnet_amd import Trainer, binding as B  # noqa: E402
from resnet_amd.trainer import resnet_dims  # noqa: E402

HAS_DEVICE_HEAD = "mi_trainer_set_loss" in B.PROTOTYPES
DEVICE_FLAGS = 1 | 2  # MI_LOSS_DEVICE | MI_LOSS_NO_PRED_COPY


def time_head(calls, warmup):
    lib = B.load()
    N, L = 256, 1000
    tr = Trainer(resnet_dims(input=32, n_conv_blocks=1, reductions=(), final_depth=256, output=L), N, device=0)
    try:
        if lib.mi_device_count() < 1:
            raise RuntimeError("bench_head needs a HIP device")
        tr.source_synthetic()
        tr.load_new_batch()
        tr.forward()
        tr.check()
        t = tr.t.contents
        fb, bb = t.forward_buffer.contents, t.backprop_buffer.contents
        vp = lambda p: C.cast(p, C.c_void_p)  # noqa: E731
        logits, labels = vp(fb.activations.contents.linear_output), vp(tr.c_batch.contents.correct_classes)
        pred, pred_cpu, deriv = vp(fb.pred), vp(fb.pred_cpu), vp(bb.output_layer_deriv)

        class MiGlobal(C.Structure):
            _fields_ = [("ready", C.c_int), ("compute", C.c_void_p)]
        lib.mi_global.restype = C.POINTER(MiGlobal)
        stream = C.c_void_p(lib.mi_global().contents.compute)
        lib.mid_softmax.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        lib.mid_ce_deriv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        lib.mid_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.mid_stream_sync.argtypes = [C.c_void_p]
        nw = C.c_int(0)

        def host_head():
            lib.mid_softmax(stream, logits, pred, N, L)
            lib.mid_memcpy_d2h(pred_cpu, pred, N * L * 4, stream)
            lib.mid_stream_sync(stream)
            lib.mi_host_loss(tr.t, C.byref(nw))
            lib.mid_ce_deriv(stream, pred, labels, deriv, N, L)
            lib.mid_stream_sync(stream)

        legs = {"a_host_head": host_head}
        if HAS_DEVICE_HEAD:
            rows, ranks, rec = lib.mi_malloc(N * 4), lib.mi_malloc(N * 4), lib.mi_malloc(2 * C.sizeof(B.MiLossMetrics))
            last = B.MiLossMetrics()

            def device_head():
                lib.mi_op_loss_head(logits, labels, pred, deriv, rows, ranks, N, L, 0.0, 5, rec, None)

            def device_head_read():
                device_head()
                lib.mi_copy_to_host(C.byref(last), rec, C.sizeof(last))

            legs["b_device_head"] = device_head
            legs["b_device_head_and_record"] = device_head_read
        for fn in legs.values():
            for _ in range(warmup):
                fn()
        ms = {k: [] for k in legs}
        for _ in range(5):  # the legs alternate in rounds of calls / 5: drift hits all alike, and no call is timed right behind another leg's
            for k, fn in legs.items():
                fn()
                for _ in range(max(calls // 5, 1)):
                    t0 = time.perf_counter()
                    fn()
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        tr.check()
        return {k: dict(ms=round(float(np.median(v)), 4), ms_min=round(float(np.min(v)), 4), ms_p90=round(float(np.percentile(v, 90)), 4)) for k, v in ms.items()}
    finally:
        tr.close()


def time_steps(dtype, batch, steps, blocks, warmup):
    lib = B.load()
    tr = Trainer(resnet_dims(), batch, lr=1e-4, seed=1236, device=0)
    try:
        if lib.mi_device_count() < 1:
            raise RuntimeError("bench_head needs a HIP device")
        if dtype == "bf16":
            tr.set_dtype(B.MI_DTYPE_BF16)
        tr.source_synthetic()

        def loop_step():
            tr.step()

        def loop_async():
            tr.load_new_batch(); tr.forward(); tr.backward(); tr.update()

        modes = {"host": (0.0, 1, 0, loop_step)}
        if HAS_DEVICE_HEAD:
            modes["device"] = (0.0, 5, DEVICE_FLAGS, loop_step)
            modes["device_async"] = (0.0, 5, DEVICE_FLAGS, loop_async)

        def block(mode, k):
            smoothing, topk, flags, one = modes[mode]
            if HAS_DEVICE_HEAD and lib.mi_trainer_set_loss(tr.t, smoothing, topk, flags) != 0:
                raise RuntimeError(tr.error())
            lib.mi_device_synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                one()
            if HAS_DEVICE_HEAD and flags:
                tr.metrics(reset=True)
            lib.mi_device_synchronize()
            dt = time.perf_counter() - t0
            tr.check()
            return dt / k * 1e3

        for mode in modes:
            block(mode, warmup)
        ms = {m: [] for m in modes}
        for _ in range(blocks):
            for mode in modes:
                ms[mode].append(block(mode, steps))
        assert tr.check_errors() == 0
        return {m: dict(ms_per_step=round(float(np.median(v)), 3), spread_ms=round(float(np.max(v) - np.min(v)), 3), blocks=[round(x, 3) for x in v])
                for m, v in ms.items()}
    finally:
        tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per mode")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per mode (head: calls per leg)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--head-calls", type=int, default=200)
    ap.add_argument("--skip-head", action="store_true")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)  # the child process of one storage type
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(time_steps(args.leg, args.batch, args.steps, args.blocks, args.warmup)))
        return
    out = {"device_head": HAS_DEVICE_HEAD, "batch": args.batch, "steps_per_block": args.steps, "blocks": args.blocks}
    if not args.skip_head:
        out["head_ms"] = time_head(args.head_calls, max(args.warmup, 10))
        for k, v in out["head_ms"].items():
            print("head %-26s %8.4f ms (min %.4f, p90 %.4f)" % (k, v["ms"], v["ms_min"], v["ms_p90"]))
    for dtype in [d for d in args.dtypes.split(",") if d]:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", dtype, "--batch", str(args.batch), "--steps", str(args.steps),
               "--blocks", str(args.blocks), "--warmup", str(args.warmup)]
        res = json.loads(subprocess.check_output(cmd).decode().strip().splitlines()[-1])
        out["step_" + dtype] = res
        for m, v in res.items():
            print("step %-4s %-13s %9.3f ms / step (spread of %d blocks %.3f ms)" % (dtype, m, v["ms_per_step"], args.blocks, v["spread_ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
