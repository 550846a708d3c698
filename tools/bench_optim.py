#!/usr/bin/env python3
"""Times one optimizer update (update_parameters) over the ResNet-50 parameter arena: Adam (the default), momentum SGD and LARS.
A ResNet-50 trainer at batch 1 on the synthetic source runs full steps; the update phase of each is timed by the trainer's own
HIP events (mi_trainer_last_timings [3]), with the per-step input reset off so that the phase holds the optimizer launches only.
Bytes are the algorithmic traffic over the arena: Adam and LARS 8 passes (LARS: w, g for the norms, then w, g, b in and out),
SGD 6.
  python tools/bench_optim.py [--steps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnet_amd import Trainer  # noqa: E402
from resnet_amd.trainer import resnet_dims  # noqa: E402

PASSES = {"adam": 8, "sgd": 6, "lars": 8}


def time_update(kind, steps, warmup):
    tr = Trainer(resnet_dims(), 1, lr=0.01 if kind != "adam" else 1e-4, wd=5e-5, device=0)
    try:
        if tr.L.mi_device_count() < 1:
            raise RuntimeError("bench_optim needs a HIP device")
        tr.set_optimizer(kind)
        tr.source_synthetic()
        tr.L.mi_trainer_set_input_reset(tr.t, 0)
        ms = []
        for s in range(warmup + steps):
            tr.step()
            tr.check()
            if s >= warmup:
                ms.append(tr.timings()[3])  # waits for the compute stream
        assert tr.check_errors() == 0
        arena = sum(tr.sizes) * 4
        return float(np.median(ms)), float(np.min(ms)), arena
    finally:
        tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    out = {}
    for kind in ("adam", "sgd", "lars"):
        med, best, arena = time_update(kind, args.steps, args.warmup)
        gbs = PASSES[kind] * arena / (med * 1e-3) / 1e9
        out[kind] = dict(ms=round(med, 4), ms_min=round(best, 4), gb_per_s=round(gbs, 1), bytes=PASSES[kind] * arena)
        print("%-5s %8.4f ms (min %.4f)  %7.1f GB/s  (%d passes over %.1f MB)" % (kind, med, best, gbs, PASSES[kind], arena / 1e6))
    out["lars_over_adam"] = round(out["lars"]["ms"] / out["adam"]["ms"], 3)
    out["sgd_over_adam"] = round(out["sgd"]["ms"] / out["adam"]["ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
