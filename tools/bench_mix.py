#!/usr/bin/env python3
"""What mixup / CutMix cost (mi_trainer_set_mix, include/resnet_mi.h "mixing").

  mix    mi_op_mix_batch on a batch of 256 x 3 x 224 x 224 floats (154 MB) in device memory: mixup (every element of every pair read and
         written once: 2 x 154 MB of traffic), CutMix with a centred box of half the image's area and with the whole image.  ms per call,
         host clock around a call that ends in a stream synchronise, median / minimum over the calls; GB/s = bytes read + written / median.
  head   mi_op_loss_head against mi_op_loss_head_mix (lam 0.3) at N = 256, L = 1000, smoothing 0.1, the legs alternating in rounds.
  step   ResNet-50 at batch 256 from the synthetic source, one process per storage type, ONE trainer with the device head
         (MI_LOSS_DEVICE | MI_LOSS_NO_PRED_COPY, smoothing 0.1) whose mixing is switched off and on between blocks of steps, alternating
         so that drift hits both alike.  ms per step = block time / steps from a device synchronise to a device synchronise; per mode
         the median over the blocks and their spread (max - min).

  python tools/bench_mix.py [--steps 10] [--blocks 5] [--warmup 5] [--batch 256] [--calls 100] [--skip-ops] [--dtypes f32,bf16]
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
        raise RuntimeError("bench_mix needs a HIP device")
    D = 224
    size = 3 * D * D
    images = lib.mi_malloc(batch * size * 4)
    assert images and lib.mi_op_fill_uniform(images, batch * size, 1234, -124.0, 152.0) == 0, lib.mi_last_error()
    half = int(round(D * (0.5 ** 0.5)))
    lo = (D - half) // 2
    plans = {"mixup": (B.MiMixPlan(1, 0.3, 0, 0, 0, 0), size), "cutmix_half": (B.MiMixPlan(2, 0.5, lo, lo, lo + half, lo + half), 3 * half * half),
             "cutmix_whole": (B.MiMixPlan(2, 0.0, 0, 0, D, D), size)}
    legs = {k: (lambda p=p: lib.mi_op_mix_batch(images, batch, size, D, C.byref(p))) for k, (p, _) in plans.items()}
    out = {}
    for k, (ms, ms_min) in _time(legs, calls, warmup).items():
        traffic = 2 * (batch // 2) * plans[k][1] * 4 * 2  # both images of every pair, read and written
        out["mix_" + k] = dict(ms=round(ms, 4), ms_min=round(ms_min, 4), gb_per_s=round(traffic / ms * 1e-6, 1), mb=round(traffic * 1e-6, 1))
    lib.mi_free(images)
    N, L = 256, 1000
    rng = np.random.RandomState(0)

    def dev(a):
        p = lib.mi_malloc(a.nbytes)
        lib.mi_copy_to_device(p, a.ctypes.data, a.nbytes)
        return p

    x = dev((3 * rng.randn(N, L)).astype(np.float32))
    la, lb = dev(rng.randint(0, L, N).astype(np.int32)), dev(rng.randint(0, L, N).astype(np.int32))
    pred, dl, rows, ranks = (lib.mi_malloc(n) for n in (N * L * 4, N * L * 4, N * 4, N * 4))
    rec = dev(np.zeros(C.sizeof(B.MiLossMetrics), np.uint8))
    legs = {"head_one_label": lambda: lib.mi_op_loss_head(x, la, pred, dl, rows, ranks, N, L, 0.1, 5, rec, None),
            "head_two_labels": lambda: lib.mi_op_loss_head_mix(x, la, lb, 0.3, pred, dl, rows, ranks, N, L, 0.1, 5, rec, None)}
    for k, (ms, ms_min) in _time(legs, calls, warmup).items():
        out[k] = dict(ms=round(ms, 4), ms_min=round(ms_min, 4))
    if lib.mi_last_error():
        raise RuntimeError(lib.mi_last_error().decode())
    return out


def time_steps(dtype, batch, steps, blocks, warmup):
    lib = B.load()
    tr = Trainer(resnet_dims(), batch, lr=1e-4, seed=1236, device=0)
    try:
        if lib.mi_device_count() < 1:
            raise RuntimeError("bench_mix needs a HIP device")
        if dtype == "bf16":
            tr.set_dtype(B.MI_DTYPE_BF16)
        tr.source_synthetic()
        tr.set_loss(smoothing=0.1, topk=5, device=True, copy_pred=False)
        modes = {"mix_off": dict(mixup=0.0, cutmix=0.0), "mix_on": dict(mixup=0.2, cutmix=1.0, prob=1.0, switch=0.5, seed=1)}

        def block(mode, k):
            tr.set_mix(**modes[mode])
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
            print("%-18s %8.4f ms (min %.4f)%s" % (k, v["ms"], v["ms_min"], "  %7.1f GB/s of %.1f MB" % (v["gb_per_s"], v["mb"]) if "mb" in v else ""))
    for dtype in [d for d in args.dtypes.split(",") if d]:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", dtype, "--batch", str(args.batch), "--steps", str(args.steps),
               "--blocks", str(args.blocks), "--warmup", str(args.warmup)]
        res = json.loads(subprocess.check_output(cmd).decode().strip().splitlines()[-1])
        out["step_" + dtype] = res
        for m, v in res.items():
            print("step %-4s %-8s %9.3f ms / step (spread of %d blocks %.3f ms)" % (dtype, m, v["ms_per_step"], args.blocks, v["spread_ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
