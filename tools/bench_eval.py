#!/usr/bin/env python3
"""What evaluation costs (include/resnet_mi.h, "evaluation"): ResNet-50 at batch 256 from the synthetic source, one process per storage
type, ONE trainer whose settings are switched between blocks of steps, the modes alternating block by block so that drift hits all alike.

  track   the training step with mi_trainer_track_running_stats off and on (one extra launch over 26 560 channels per forward_pass),
          and "off_again": the first mode a second time in every round -- two legs of identical work, whose difference is what the
          measurement itself cannot tell apart.  ms per step = block time / steps, host clock from a device synchronise to a device
          synchronise; per mode the median over the blocks and the spread (max - min) of its blocks.
  eval    mi_trainer_eval_forward on the current batch, ms per pass (a block of passes between two device synchronises) and images/s,
          beside the forward phase of the training steps just timed (mi_trainer_last_timings[1], device events, median over the steps of
          the tracking-on blocks).  The training forward ends in the copy of pred and a stream synchronise; the eval pass in neither.

  python tools/bench_eval.py [--steps 10] [--blocks 5] [--warmup 5] [--batch 256] [--dtypes f32,bf16]
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


def run(dtype, batch, steps, blocks, warmup):
    lib = B.load()
    tr = Trainer(resnet_dims(), batch, lr=1e-4, seed=1236, device=0)
    try:
        if lib.mi_device_count() < 1:
            raise RuntimeError("bench_eval needs a HIP device")
        if dtype == "bf16":
            tr.set_dtype(B.MI_DTYPE_BF16)
        tr.source_synthetic()
        fwd_ms = []

        def train_block(on, k, keep_fwd=False):
            tr.track_running_stats(0.1, on=on)
            lib.mi_device_synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                tr.step()
                if keep_fwd:
                    fwd_ms.append(tr.timings()[1])  # (waits for the step: the same in every block of this mode)
            lib.mi_device_synchronize()
            dt = time.perf_counter() - t0
            tr.check()
            return dt / k * 1e3

        def eval_block(k):
            tr.track_running_stats(0.1, on=True)
            tr.load_new_batch()
            lib.mi_device_synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                tr.eval_forward()
            lib.mi_device_synchronize()
            dt = time.perf_counter() - t0
            tr.check()
            return dt / k * 1e3

        modes = {"off": lambda k: train_block(False, k), "on": lambda k: train_block(True, k, True), "off_again": lambda k: train_block(False, k),
                 "eval": eval_block}
        for fn in modes.values():
            fn(warmup)
        del fwd_ms[:]
        ms = {m: [] for m in modes}
        for _ in range(blocks):
            for m, fn in modes.items():
                ms[m].append(fn(steps))
        assert tr.check_errors() == 0
        out = {m: dict(ms=round(float(np.median(v)), 3), spread_ms=round(float(np.max(v) - np.min(v)), 3), blocks=[round(x, 3) for x in v])
               for m, v in ms.items()}
        f = float(np.median(fwd_ms))
        out["train_forward"] = dict(ms=round(f, 3), images_per_s=round(batch / f * 1e3, 1))
        out["eval"]["images_per_s"] = round(batch / out["eval"]["ms"] * 1e3, 1)
        out["running_updates"] = tr.running_updates()
        return out
    finally:
        tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="steps (eval: passes) per timed block")
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per mode")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per mode")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)  # the child process of one storage type
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(run(args.leg, args.batch, args.steps, args.blocks, args.warmup)))
        return
    out = {"batch": args.batch, "steps_per_block": args.steps, "blocks": args.blocks}
    for dtype in [d for d in args.dtypes.split(",") if d]:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", dtype, "--batch", str(args.batch), "--steps", str(args.steps),
               "--blocks", str(args.blocks), "--warmup", str(args.warmup)]
        res = json.loads(subprocess.check_output(cmd).decode().strip().splitlines()[-1])
        out[dtype] = res
        for m in ("off", "on", "off_again"):
            print("%-4s step, tracking %-9s %9.3f ms / step (spread of %d blocks %.3f ms)" % (dtype, m, res[m]["ms"], args.blocks, res[m]["spread_ms"]))
        print("%-4s eval_forward            %9.3f ms / pass = %.1f images/s (spread %.3f ms); training forward phase %.3f ms = %.1f images/s"
              % (dtype, res["eval"]["ms"], res["eval"]["images_per_s"], res["eval"]["spread_ms"], res["train_forward"]["ms"],
                 res["train_forward"]["images_per_s"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
