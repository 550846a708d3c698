#!/usr/bin/env python3
"""What TrivialAugmentWide costs (mi_trainer_set_trivial_augment, include/resnet_mi.h "TrivialAugmentWide").

  ops    mi_op_trivial_augment on a batch of 256 x 3 x 224 x 224 floats in device memory: the records of mi_ta_plan (a mix of the 14
         operations, as a step draws them), then every row under one operation family alone (table without statistics, table with
         statistics, Color, Sharpness, the gather).  ms per call, host clock around a call that ends in a stream synchronise (the memset of
         the statistics and the stage and apply launches of every 128 rows included), median / minimum over the calls; GB/s = algorithmic
         bytes / median, 30 bytes per pixel of a row with an operation (12 read + 3 written by the stage pass, 3 read + 12 written by the
         apply pass).
  step   ResNet-50 at batch 256 from the synthetic source, one process per storage type, ONE trainer with the device head
         (MI_LOSS_DEVICE | MI_LOSS_NO_PRED_COPY, smoothing 0.1) whose transform is switched off and on between blocks of steps,
         alternating so that drift hits both alike.  ms per step = block time / steps from a device synchronise to a device
         synchronise; per mode the median over the blocks and their spread (max - min).

  python tools/bench_ta.py [--steps 10] [--blocks 5] [--warmup 5] [--batch 256] [--calls 50] [--skip-ops] [--dtypes f32,bf16]
"""
import argparse
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

FAMILIES = {"table_posterize": (10, 20, 0), "table_equalize": (13, 0, 0), "table_contrast": (8, 20, 0), "color": (7, 20, 1),
            "sharpness": (9, 30, 0), "gather_rotate": (5, 7, 1), "gather_shear_x": (1, 30, 0)}


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
        raise RuntimeError("bench_ta needs a HIP device")
    D = 224
    size = 3 * D * D
    images = lib.mi_malloc(batch * size * 4)
    work = lib.mi_malloc(lib.mi_ta_workspace_bytes(batch, D))
    assert images and work and lib.mi_op_fill_uniform(images, batch * size, 1234, -124.0, 152.0) == 0, lib.mi_last_error()
    legs, active = {}, {}
    plan = (B.MiTaRow * batch)()
    assert lib.mi_ta_plan(1, 0, 0, 0, 1, batch, D, plan) == 0
    sets = {"plan_mix": plan}
    for name, (op, b, neg) in FAMILIES.items():
        rows = (B.MiTaRow * batch)()
        for i in range(batch):
            assert lib.mi_ta_row(op, b, neg, D, rows[i]) == 0
        sets[name] = rows
    for name, rows in sets.items():
        legs[name] = lambda r=rows: lib.mi_op_trivial_augment(images, batch, size, D, r, work)
        active[name] = sum(rows[i].op != 0 for i in range(batch))
    out = {}
    for k, (ms, ms_min) in _time(legs, calls, warmup).items():
        nbytes = 30.0 * active[k] * D * D
        out[k] = dict(ms=round(ms, 4), ms_min=round(ms_min, 4), gb_per_s=round(nbytes / ms * 1e-6, 1), mb=round(nbytes * 1e-6, 2), rows=active[k])
    lib.mi_free(images)
    lib.mi_free(work)
    if lib.mi_last_error():
        raise RuntimeError(lib.mi_last_error().decode())
    return out


def time_steps(dtype, batch, steps, blocks, warmup):
    lib = B.load()
    tr = Trainer(resnet_dims(), batch, lr=1e-4, seed=1236, device=0)
    try:
        if lib.mi_device_count() < 1:
            raise RuntimeError("bench_ta needs a HIP device")
        if dtype == "bf16":
            tr.set_dtype(B.MI_DTYPE_BF16)
        tr.source_synthetic()
        tr.set_loss(smoothing=0.1, topk=5, device=True, copy_pred=False)
        modes = {"ta_off": dict(on=False), "ta_on": dict(on=True, seed=1)}

        def block(mode, k):
            tr.set_trivial_augment(**modes[mode])
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
    ap.add_argument("--calls", type=int, default=50)
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
            print("%-16s %8.4f ms (min %.4f)  %7.1f GB/s of %.2f MB in %d rows" % (k, v["ms"], v["ms_min"], v["gb_per_s"], v["mb"], v["rows"]))
    for dtype in [d for d in args.dtypes.split(",") if d]:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", dtype, "--batch", str(args.batch), "--steps", str(args.steps),
               "--blocks", str(args.blocks), "--warmup", str(args.warmup)]
        res = json.loads(subprocess.check_output(cmd).decode().strip().splitlines()[-1])
        out["step_" + dtype] = res
        for m, v in res.items():
            print("step %-4s %-7s %9.3f ms / step (spread of %d blocks %.3f ms)" % (dtype, m, v["ms_per_step"], args.blocks, v["spread_ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
