#!/usr/bin/env python3
"""What random erasing costs (mi_trainer_set_erase, include/resnet_mi.h "random erasing").

  erase  mi_op_erase_batch on a batch of 256 x 3 x 224 x 224 floats in device memory, the boxes drawn by mi_erase_plan at prob 0.1 (what the
         recipes use) and 1.0 (every row), both fill modes.  ms per call, host clock around a call that ends in a stream synchronise (the
         launch, or the two at a batch above 256, included), median / minimum over the calls; GB/s = bytes written / median.
  step   ResNet-50 at batch 256 from the synthetic source, one process per storage type, ONE trainer with the device head
         (MI_LOSS_DEVICE | MI_LOSS_NO_PRED_COPY, smoothing 0.1) whose erasing is switched off and on (prob 0.1, noise) between blocks of
         steps, alternating so that drift hits both alike.  ms per step = block time / steps from a device synchronise to a device
         synchronise; per mode the median over the blocks and their spread (max - min).

  python tools/bench_erase.py [--steps 10] [--blocks 5] [--warmup 5] [--batch 256] [--calls 100] [--skip-ops] [--dtypes f32,bf16]
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

SCALE, RATIO = (0.02, 0.33), (0.3, 3.3)


def _time(legs, calls, warmup):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in legs}
    for _ in range(5):
        for k, fn in legs.items():
            fn()
            for _ in range(max(calls // 5, 1)):
                t0 = time.perf_counter()
                fn()
                ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in ms.items()}


def time_ops(batch, calls, warmup):
    lib = B.load()
    if lib.mi_device_count() < 1:
        raise RuntimeError("bench_erase needs a HIP device")
    D = 224
    size = 3 * D * D
    images = lib.mi_malloc(batch * size * 4)
    assert images and lib.mi_op_fill_uniform(images, batch * size, 1234, -124.0, 152.0) == 0, lib.mi_last_error()
    legs, written = {}, {}
    for prob in (0.1, 1.0):
        boxes = np.zeros((batch, 4), np.int32)
        assert lib.mi_erase_plan(1, 0, 0, 0, 1, batch, D, prob, SCALE[0], SCALE[1], RATIO[0], RATIO[1], boxes.ctypes.data) == 0
        for mode in ("const", "noise"):
            fill = B.erase_fill_struct(mode, (0, 0, 0), (58.395, 57.12, 57.375), 7)
            key = "erase_%s_p%g" % (mode, prob)
            legs[key] = lambda b=boxes, f=fill: lib.mi_op_erase_batch(images, batch, size, D, b.ctypes.data, C.byref(f), 0)
            written[key] = (int(np.sum(boxes[:, 2].astype(np.int64) * boxes[:, 3])) * 12, int(np.sum(boxes[:, 2] * boxes[:, 3] > 0)))
    out = {}
    for k, (ms, ms_min) in _time(legs, calls, warmup).items():
        out[k] = dict(ms=round(ms, 4), ms_min=round(ms_min, 4), gb_per_s=round(written[k][0] / ms * 1e-6, 1), mb=round(written[k][0] * 1e-6, 2),
                      rows_erased=written[k][1])
    lib.mi_free(images)
    if lib.mi_last_error():
        raise RuntimeError(lib.mi_last_error().decode())
    return out


def time_steps(dtype, batch, steps, blocks, warmup):
    lib = B.load()
    tr = Trainer(resnet_dims(), batch, lr=1e-4, seed=1236, device=0)
    try:
        if lib.mi_device_count() < 1:
            raise RuntimeError("bench_erase needs a HIP device")
        if dtype == "bf16":
            tr.set_dtype(B.MI_DTYPE_BF16)
        tr.source_synthetic()
        tr.set_loss(smoothing=0.1, topk=5, device=True, copy_pred=False)
        modes = {"erase_off": dict(prob=0.0), "erase_on": dict(prob=0.1, mode="noise", seed=1)}

        def block(mode, k):
            tr.set_erase(**modes[mode])
            lib.mi_device_synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                tr.load_new_batch(); tr.forward(); tr.backward(); tr.update()
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
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per mode (operators: calls per leg)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--skip-ops", action="store_true")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)  # the child process of one storage type
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(time_steps(args.leg, args.batch, args.steps, args.blocks, args.warmup)))
        return
    out = {"batch": args.batch, "steps_per_block": args.steps, "blocks": args.blocks}
    if not args.skip_ops:
        out["ops"] = time_ops(args.batch, args.calls, max(args.warmup, 10))
        for k, v in out["ops"].items():
            print("%-18s %8.4f ms (min %.4f)  %7.1f GB/s of %.2f MB in %d rows" % (k, v["ms"], v["ms_min"], v["gb_per_s"], v["mb"], v["rows_erased"]))
    for dtype in [d for d in args.dtypes.split(",") if d]:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", dtype, "--batch", str(args.batch), "--steps", str(args.steps),
               "--blocks", str(args.blocks), "--warmup", str(args.warmup)]
        res = json.loads(subprocess.check_output(cmd).decode().strip().splitlines()[-1])
        out["step_" + dtype] = res
        for m, v in res.items():
            print("step %-4s %-9s %9.3f ms / step (spread of %d blocks %.3f ms)" % (dtype, m, v["ms_per_step"], args.blocks, v["spread_ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
