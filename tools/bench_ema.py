#!/usr/bin/env python3
"""Times weight averaging (mi_trainer_set_ema, include/resnet_mi.h) on the ResNet-50 arena.

kernels   one EMA update (3 passes of algorithmic traffic over the arena: e and p in, e out) and one exchange (4 passes) through the
          operator layer on two device arrays of the arena's size, each launch bracketed by HIP events on its stream (mi_prof_*); beside
          them, from the same run, the update phase of a ResNet-50 trainer with momentum SGD (6 passes; tools/bench_optim.py's number)
          with the EMA off and at every=1, timed by the trainer's own events (mi_trainer_last_timings [3])
step      the ResNet-50 training step at batch 256, bf16 and fp32, with the EMA off, every=1 and every=32: wall clock over --steps steps
          behind --warmup, the device drained at both ends
eval      mi_trainer_eval_forward at batch 256 (bf16) on the raw and on the averaged model (two exchanges per call)
  python tools/bench_ema.py [--steps 64] [--warmup 5] [--batch 256]"""
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
    a, b = ops.dev(rng.randn(n).astype(np.float32)), ops.dev(rng.randn(n).astype(np.float32))
    out = {}
    for name, passes, call in (("ema_update", 3, lambda: L.mi_op_ema_update(a.ptr, b.ptr, n, 1e-4)), ("exchange", 4, lambda: L.mi_op_exchange(a.ptr, b.ptr, n))):
        for _ in range(3):
            assert call() == 0, L.mi_last_error()
        L.mi_prof_enable(1 << FAM_OTHER)
        L.mi_prof_reset()
        for _ in range(reps):
            assert call() == 0, L.mi_last_error()
        launches, ms, by = C.c_long(0), C.c_double(0), C.c_double(0)
        L.mi_prof_get(FAM_OTHER, C.byref(launches), C.byref(ms), None, C.byref(by))
        L.mi_prof_enable(0)
        assert launches.value == reps and by.value == passes * 4.0 * n * reps
        per = ms.value / reps
        out[name] = dict(ms=round(per, 4), gb_per_s=round(passes * 4.0 * n / (per * 1e-3) / 1e9, 1), passes=passes)
        print("%-10s %8.4f ms  %7.1f GB/s  (%d passes over %.1f MB)" % (name, per, out[name]["gb_per_s"], passes, 4.0 * n / 1e6))
    a.free(); b.free()
    return out


def update_phase(ema, steps, warmup):
    """tools/bench_optim.py's measurement of the SGD update, with and without the EMA launches behind it"""
    tr = Trainer(resnet_dims(), 1, lr=0.01, wd=5e-5, device=0)
    try:
        tr.set_optimizer("sgd")
        tr.source_synthetic()
        tr.L.mi_trainer_set_input_reset(tr.t, 0)
        tr.track_running_stats(0.1)
        if ema:
            tr.set_ema(0.9999, every=1)
        ms = []
        for s in range(warmup + steps):
            tr.step()
            tr.check()
            if s >= warmup:
                ms.append(tr.timings()[3])
        assert tr.check_errors() == 0
        return float(np.median(ms))
    finally:
        tr.close()


def step_ms(dtype, batch, every, steps, warmup):
    tr = Trainer(resnet_dims(), batch, lr=0.01, wd=5e-5, device=0)
    try:
        tr.set_dtype(dtype)
        tr.set_optimizer("sgd")
        tr.set_loss(smoothing=0.1, device=True, copy_pred=False)
        tr.source_synthetic()
        tr.track_running_stats(0.1)
        if every:
            tr.set_ema(0.9999, every=every)
        for _ in range(warmup):
            tr.step()
        tr.L.mi_device_synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.load_new_batch(); tr.forward(); tr.backward(); tr.update()
        tr.L.mi_device_synchronize()
        dt = (time.perf_counter() - t0) * 1e3 / steps
        assert tr.check_errors() == 0 and (not every or tr.ema_updates() == (warmup + steps) // every)
        return dt
    finally:
        tr.close()


def eval_ms(batch, steps, warmup):
    tr = Trainer(resnet_dims(), batch, device=0)
    try:
        tr.set_dtype(B.MI_DTYPE_BF16)
        tr.source_synthetic()
        tr.track_running_stats(0.1)
        tr.step()
        tr.set_ema(0.9999, every=1)
        tr.load_new_batch()
        out = {}
        for name, on in (("raw", False), ("ema", True)):
            tr.eval_use_ema(on)
            for _ in range(warmup):
                tr.eval_forward()
            tr.L.mi_device_synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.eval_forward()
            tr.L.mi_device_synchronize()
            out[name] = (time.perf_counter() - t0) * 1e3 / steps
        tr.check()
        return out
    finally:
        tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", choices=["kernels", "step", "eval"], default=None)
    args = ap.parse_args()
    ops = Ops()
    if ops.L.mi_device_count() < 1:
        raise RuntimeError("bench_ema needs a HIP device")
    dims = resnet_dims()
    c_flags = (C.c_int * dims["n_conv_blocks"])(*dims["is_block_spatial_reduction"])
    c_dims = ops.L.init_dimensions(dims["input"], 7, dims["init_conv_filters"], 2, 3, 2, dims["n_conv_blocks"], c_flags, dims["final_depth"], dims["output"])
    arena = int(ops.L.mi_debug_arena_floats(c_dims))
    out = {"arena_floats": arena}
    if args.only in (None, "kernels"):
        out["kernels"] = kernels(ops, arena, 50)
        sgd, both = update_phase(False, args.steps, args.warmup), update_phase(True, args.steps, args.warmup)
        out["update_phase_ms"] = dict(sgd=round(sgd, 4), sgd_and_ema=round(both, 4))
        print("update phase (trainer events): SGD %.4f ms (6 passes), SGD + EMA of parameters and running statistics %.4f ms" % (sgd, both))
    if args.only in (None, "step"):
        out["step_ms"] = {}
        for name, dt in (("bf16", B.MI_DTYPE_BF16), ("fp32", B.MI_DTYPE_F32)):
            row = {("off" if not e else "every%d" % e): round(step_ms(dt, args.batch, e, args.steps, args.warmup), 3) for e in (0, 1, 32)}
            out["step_ms"][name] = row
            print("step %s batch %d: EMA off %.3f ms, every=1 %.3f ms (%+.2f%%), every=32 %.3f ms (%+.2f%%)" % (
                name, args.batch, row["off"], row["every1"], 100 * (row["every1"] / row["off"] - 1), row["every32"], 100 * (row["every32"] / row["off"] - 1)))
    if args.only in (None, "eval"):
        ev = eval_ms(args.batch, args.steps, args.warmup)
        out["eval_forward_ms"] = {k: round(v, 3) for k, v in ev.items()}
        print("eval_forward bf16 batch %d: raw %.3f ms, averaged model %.3f ms" % (args.batch, ev["raw"], ev["ema"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
