#!/usr/bin/env python3
"""Times gradient clipping (mi_trainer_set_clip_grad_norm, include/resnet_mi.h) on the ResNet-50 arena.

kernels   the three launches on their own over the ResNet-50 tensors (mi_debug_clip_pass_ms: each launch between HIP events on its
          stream, the mean over --reps behind 3 unmeasured ones): the norm (reads 4 bytes per parameter), the coefficient (8 bytes per
          chunk), the scale clipped (reads and writes 4 bytes per parameter) and the scale unclipped (the early exit: one word per
          workgroup); GB/s over those algorithmic bytes
update    the update phase of a ResNet-50 trainer at batch 1 (tools/bench_optim.py's measurement: the trainer's own events,
          mi_trainer_last_timings [3]) for Adam and LARS with clipping off, on and clipping at every step, on and never clipping
step      the ResNet-50 training step at --batch (bf16 and fp32, Adam and LARS) with clipping off / on (clipping at every step): wall
          clock over --steps steps behind --warmup, the device drained at both ends, the two settings alternating --rounds times
  python tools/bench_clip.py [--steps 32] [--warmup 5] [--batch 256] [--reps 50] [--only kernels|update|step]"""
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

CHUNK = 8192
TINY, HUGE = 1e-3, 1e30  # max_norm that clips every gradient here / none


def r50_offsets():
    tr = Trainer(resnet_dims(), 1, device=0)
    try:
        return np.concatenate([[0], np.cumsum(tr.sizes)]).astype(np.uint64)  # ResNet-50 has no alignment padding
    finally:
        tr.close()


def kernels(ops, off, reps):
    L = ops.L
    n = int(off[-1])
    chunks = int(sum((int(b) - int(a) + CHUNK - 1) // CHUNK for a, b in zip(off[:-1], off[1:])))
    g = ops.dev(np.random.RandomState(0).randn(n).astype(np.float32))
    out = {"chunks": chunks}
    # the clipped scale multiplies g by coef reps + 3 times: a coef close to 1 (max_norm just below the norm) keeps the values in range
    norm = float(np.sqrt(n))
    for name, which, max_norm, nbytes in (("norm", 0, HUGE, 4.0 * n), ("coef", 1, HUGE, 8.0 * chunks), ("scale_unclipped", 2, HUGE, 4.0 * chunks),
                                          ("scale_clipped", 2, 0.999 * norm, 8.0 * n)):
        ms = L.mi_debug_clip_pass_ms(which, g.ptr, n, off.ctypes.data, len(off) - 1, max_norm, reps)
        assert ms >= 0, L.mi_last_error()
        out[name] = dict(ms=round(ms, 5), gb_per_s=round(nbytes / (ms * 1e-3) / 1e9, 1), bytes=nbytes)
        print("%-16s %9.5f ms  %8.1f GB/s  (%.2f MB)" % (name, ms, out[name]["gb_per_s"], nbytes / 1e6))
    assert np.all(np.isfinite(g.get()))
    g.free()
    return out


def update_phase(kind, max_norm, steps, warmup):
    tr = Trainer(resnet_dims(), 1, lr=0.01 if kind != "adam" else 1e-4, wd=5e-5, device=0)
    try:
        tr.set_optimizer(kind)
        tr.source_synthetic()
        tr.L.mi_trainer_set_input_reset(tr.t, 0)
        tr.set_clip_grad_norm(max_norm)
        ms = []
        for s in range(warmup + steps):
            tr.step()
            tr.check()
            if s >= warmup:
                ms.append(tr.timings()[3])
        assert tr.check_errors() == 0
        if max_norm:
            rec = tr.last_clip()
            assert rec["updates"] == warmup + steps and rec["clipped"] == (warmup + steps if max_norm == TINY else 0), rec
        return float(np.median(ms))
    finally:
        tr.close()


def step_ms(dtype, kind, batch, max_norm, steps, warmup, rounds):
    """[off, on] ms per step, the two settings alternating in one trainer (the setter is legal between updates)"""
    tr = Trainer(resnet_dims(), batch, lr=0.01 if kind != "adam" else 1e-4, wd=5e-5, device=0)
    try:
        tr.set_dtype(dtype)
        tr.set_optimizer(kind)
        tr.set_loss(smoothing=0.1, device=True, copy_pred=False)
        tr.source_synthetic()
        best = [None, None]
        for _ in range(rounds):
            for i, m in enumerate((0.0, max_norm)):
                tr.set_clip_grad_norm(m)
                for _ in range(warmup):
                    tr.step()
                tr.L.mi_device_synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    tr.load_new_batch(); tr.forward(); tr.backward(); tr.update()
                tr.L.mi_device_synchronize()
                dt = (time.perf_counter() - t0) * 1e3 / steps
                best[i] = dt if best[i] is None else min(best[i], dt)
        assert tr.check_errors() == 0
        return best
    finally:
        tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--only", choices=["kernels", "update", "step"], default=None)
    args = ap.parse_args()
    ops = Ops()
    if ops.L.mi_device_count() < 1:
        raise RuntimeError("bench_clip needs a HIP device")
    off = r50_offsets()
    out = {"arena_floats": int(off[-1])}
    if args.only in (None, "kernels"):
        out["kernels"] = kernels(ops, off, args.reps)
    if args.only in (None, "update"):
        out["update_phase_ms"] = {}
        for kind in ("adam", "lars"):
            row = {name: round(update_phase(kind, m, args.steps, args.warmup), 4) for name, m in (("off", 0.0), ("clipping", TINY), ("not_clipping", HUGE))}
            out["update_phase_ms"][kind] = row
            print("update phase %-4s: clipping off %.4f ms, on and clipping %.4f ms, on and not clipping %.4f ms" % (kind, row["off"], row["clipping"], row["not_clipping"]))
    if args.only in (None, "step"):
        out["step_ms"] = {}
        for dname, dt in (("bf16", B.MI_DTYPE_BF16), ("fp32", B.MI_DTYPE_F32)):
            for kind in ("adam", "lars"):
                off_ms, on_ms = step_ms(dt, kind, args.batch, TINY, args.steps, args.warmup, args.rounds)
                out["step_ms"]["%s_%s" % (dname, kind)] = dict(off=round(off_ms, 3), on=round(on_ms, 3))
                print("step %s %-4s batch %d: clipping off %.3f ms, on %.3f ms (%+.2f%%)" % (dname, kind, args.batch, off_ms, on_ms, 100 * (on_ms / off_ms - 1)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
