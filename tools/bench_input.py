#!/usr/bin/env python3
"""The input side of the step, measured (DESIGN.md section 7 holds the output).

1. The decode kernel of the uint8 shards (mi_op_decode_u8: crop, flip, B,G,R -> R,G,B planes, mean subtraction) at N = 256,
   256 -> 224, a RANDOM plan with flips, against the device pass of the fp32 NHWC shard path (mi_op_nhwc_to_nchw at 256 x 224^2 x 3)
   in the same run: each launch bracketed by HIP events on its stream (mi_prof family 4), the two kernels alternating, median of
   --runs launches after warm-up.  GB/s over the algorithmic bytes: decode N dim_out^2 (3 + 12), re-layout N dim_out^2 3 (4 + 4).
   Beside them the resample kernel of the random-resized crop (mi_op_resample_u8) on the boxes mi_augment_plan_rrc draws with the
   default bounds (scale 0.08 .. 1, ratio 3/4 .. 4/3): its bytes are the boxes' 3 h w in and the same 12 N dim_out^2 out.
   Then the antialiased kernel (mi_op_resample_aa_u8) beside the bilinear one, alternating, at 256 -> 224 and 256 -> 176, on
   whole-image boxes (the strongest downscale) and on the RRC plan's boxes: same bytes, so the ratio of the two is the price of the filter.
2. The whole training step on the real data path: ResNet-50 at batch 256, fp32 and bf16 storage, from (a) the synthetic pool resident
   in HBM, (b) fp32 NCHW shards with prefetch, (c) uint8 shards, RANDOM crops with flips, with prefetch, (d) the same uint8 shard
   with random-resized crops (u8 rrc), (e) the same with antialias on (u8 rrc aa).  Both shards are built from the same seeded class
   files in a temporary directory; one shard holds every timed step, so no step reads a file.  Legs (b) to (e) run three times each,
   alternating, which gives every leg the run-to-run spread the comparisons are read against: (c) against (b), (d) against (c); (e) is
   reported beside (d), no threshold is set for it.
3. Host and device bytes of the two shard sources.
  python tools/bench_input.py [--runs 30] [--steps 16] [--warmup 3] [--skip-steps]
Exit status 1 if the decode is slower than the re-layout, the uint8 leg slower than the fp32-shard leg by more than that spread, or
the rrc leg slower than the uint8 RANDOM leg by more than the RANDOM leg's own spread."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from resnet_amd import Trainer  # noqa: E402
from resnet_amd import binding as B  # noqa: E402
from resnet_amd.ops import Ops  # noqa: E402
from resnet_amd.trainer import resnet_dims  # noqa: E402

N, DIM_IN, DIM_OUT = 256, 256, 224
HBM_ACHIEVABLE = 6.3e12
FAMILY = 4  # the input-side passes


def family_ms(L):
    n, ms = C.c_long(0), C.c_double(0)
    L.mi_prof_get(FAMILY, C.byref(n), C.byref(ms), None, None)
    assert n.value == 1, n.value
    return ms.value


def bench_kernels(runs, warmup=3):
    ops = Ops()
    L = ops.L
    rng = np.random.default_rng(0)
    src = ops.dev(rng.integers(0, 256, size=(N, DIM_IN, DIM_IN, 3), dtype=np.uint8))
    plan = np.empty((N, 3), np.int32)
    assert L.mi_augment_plan(B.MI_AUG_RANDOM, 1, 7, 0, 0, N, DIM_IN, DIM_OUT, None, plan.ctypes.data) == 0
    dplan = ops.dev(plan)
    boxes = np.empty((N, 5), np.int32)
    assert L.mi_augment_plan_rrc(1, 7, 0, 0, N, DIM_IN, 0.08, 1.0, 3 / 4, 4 / 3, boxes.ctypes.data) == 0
    dboxes = ops.dev(boxes)
    out = ops.dev(shape=(N, 3, DIM_OUT, DIM_OUT))
    nhwc = ops.dev(shape=(N, DIM_OUT, DIM_OUT, 3))
    assert L.mi_op_fill_uniform(nhwc.ptr, N * DIM_OUT * DIM_OUT * 3, 1234, -124.0, 152.0) == 0
    legs = {"decode_u8": lambda: L.mi_op_decode_u8(src.ptr, dplan.ptr, out.ptr, N, DIM_IN, DIM_OUT),
            "resample_u8": lambda: L.mi_op_resample_u8(src.ptr, dboxes.ptr, out.ptr, N, DIM_IN, DIM_OUT),
            "nhwc_to_nchw": lambda: L.mi_op_nhwc_to_nchw(nhwc.ptr, out.ptr, N, DIM_OUT, DIM_OUT, 3)}
    ms = {k: [] for k in legs}
    L.mi_prof_enable(1 << FAMILY)
    for i in range(warmup + runs):
        for k, fn in legs.items():
            L.mi_prof_reset()
            assert fn() == 0, L.mi_last_error().decode()
            t = family_ms(L)
            if i >= warmup:
                ms[k].append(t)
    L.mi_prof_enable(0)
    px = N * DIM_OUT * DIM_OUT
    res = {}
    box_bytes = int(3 * (boxes[:, 2].astype(np.int64) * boxes[:, 3]).sum())
    for k, byt in (("decode_u8", px * 15), ("resample_u8", box_bytes + px * 12), ("nhwc_to_nchw", px * 24)):
        med = float(np.median(ms[k]))
        res[k] = dict(ms=round(med, 4), ms_min=round(float(np.min(ms[k])), 4), ms_max=round(float(np.max(ms[k])), 4), runs=len(ms[k]),
                      algorithmic_bytes=byt, gb_per_s=round(byt / (med * 1e-3) / 1e9, 1),
                      share_of_achievable_hbm=round(byt / (med * 1e-3) / HBM_ACHIEVABLE, 3))
        print("%-13s %8.4f ms (min %.4f, max %.4f; %d runs)  %7.1f GB/s = %.1f %% of 6.3 TB/s" %
              (k, med, res[k]["ms_min"], res[k]["ms_max"], len(ms[k]), res[k]["gb_per_s"], 100 * res[k]["share_of_achievable_hbm"]))
    res["resample_over_decode"] = round(res["resample_u8"]["ms"] / res["decode_u8"]["ms"], 3)
    res["resample_mean_box_side"] = round(float(np.sqrt((boxes[:, 2].astype(np.float64) * boxes[:, 3]).mean())), 1)
    res["decode_over_nhwc"] = round(res["decode_u8"]["ms"] / res["nhwc_to_nchw"]["ms"], 3)
    res["decode_le_nhwc"] = res["decode_u8"]["ms"] <= res["nhwc_to_nchw"]["ms"]
    return res


def bench_resample(runs, warmup=3):
    """the bilinear and the antialiased resample side by side: dim_out 224 and 176, whole-image and RRC-plan boxes"""
    ops = Ops()
    L = ops.L
    src = ops.dev(np.random.default_rng(0).integers(0, 256, size=(N, DIM_IN, DIM_IN, 3), dtype=np.uint8))
    rrc = np.empty((N, 5), np.int32)
    assert L.mi_augment_plan_rrc(1, 7, 0, 0, N, DIM_IN, 0.08, 1.0, 3 / 4, 4 / 3, rrc.ctypes.data) == 0
    whole = np.tile(np.array([0, 0, DIM_IN, DIM_IN, 0], np.int32), (N, 1))
    whole[::2, 4] = 1
    res = {}
    L.mi_prof_enable(1 << FAMILY)
    for D in (224, 176):
        out = ops.dev(shape=(N, 3, D, D))
        for name, boxes in (("whole", whole), ("rrc", rrc)):
            dbox = ops.dev(boxes)
            legs = {"resample_u8": lambda: L.mi_op_resample_u8(src.ptr, dbox.ptr, out.ptr, N, DIM_IN, D),
                    "resample_aa_u8": lambda: L.mi_op_resample_aa_u8(src.ptr, dbox.ptr, out.ptr, N, DIM_IN, D, D, 0, 0)}
            ms = {k: [] for k in legs}
            for i in range(warmup + runs):
                for k, fn in legs.items():
                    L.mi_prof_reset()
                    assert fn() == 0, L.mi_last_error().decode()
                    t = family_ms(L)
                    if i >= warmup:
                        ms[k].append(t)
            byt = int(3 * (boxes[:, 2].astype(np.int64) * boxes[:, 3]).sum()) + N * D * D * 12
            r = {}
            for k in legs:
                med = float(np.median(ms[k]))
                r[k] = dict(ms=round(med, 4), ms_min=round(float(np.min(ms[k])), 4), ms_max=round(float(np.max(ms[k])), 4),
                            gb_per_s=round(byt / (med * 1e-3) / 1e9, 1))
                print("%-15s 256 -> %d, %-5s boxes %8.4f ms (min %.4f, max %.4f; %d runs)  %7.1f GB/s" %
                      (k, D, name, med, r[k]["ms_min"], r[k]["ms_max"], len(ms[k]), r[k]["gb_per_s"]))
            r["algorithmic_bytes"] = byt
            r["aa_over_bilinear"] = round(r["resample_aa_u8"]["ms"] / r["resample_u8"]["ms"], 3)
            res["%d_%s" % (D, name)] = r
    L.mi_prof_enable(0)
    return res


def build_shards(root, per_shard):
    """seeded class files -> one fp32 NCHW shard and one uint8 shard of the same images (the library's two writers)"""
    L = B.load()
    rng = np.random.default_rng(1)
    n_classes = 16
    per_class = per_shard // n_classes
    data, part, f32, u8 = (os.path.join(root, d) for d in ("classes", "part", "f32", "u8"))
    for d in (data, part, f32, u8):
        os.makedirs(d)
    for c in range(n_classes):
        rng.integers(0, 256, size=per_class * DIM_IN * DIM_IN * 3, dtype=np.uint8).tofile(os.path.join(data, "%08d.buffer" % c))
    csv = os.path.join(part, "000_images.csv")
    off = rng.integers(0, DIM_IN - DIM_OUT + 1, size=(per_shard, 2))
    with open(csv, "w") as f:
        for i in range(per_shard):
            f.write("%03d,%04d,%02d,%02d\n" % (i % n_classes, i // n_classes, off[i, 0], off[i, 1]))
    assert L.mi_build_shard(csv.encode(), data.encode(), f32.encode(), 0, DIM_IN, DIM_OUT, B.MI_LAYOUT_NCHW) == per_shard
    assert L.mi_build_shard_u8(csv.encode(), data.encode(), u8.encode(), 0, DIM_IN) == per_shard
    shutil.rmtree(data)
    sizes = {d: sum(os.path.getsize(os.path.join(p, f)) for f in os.listdir(p)) for d, p in (("f32", f32), ("u8", u8))}
    return f32, u8, sizes


def time_leg(kind, dtype, dirs, per_shard, steps, warmup):
    tr = Trainer(resnet_dims(), N, lr=1e-4, seed=1236, shard_n_images=per_shard, device=0)
    try:
        if dtype == "bf16":
            tr.set_dtype(B.MI_DTYPE_BF16)
        if kind == "synthetic":
            tr.source_synthetic(1234, 1235, pool_batches=2)
        elif kind == "f32_shards":
            tr.source_shards(dirs[0], B.MI_LAYOUT_NCHW, prefetch=True)
        elif kind == "u8_rrc_aa":
            tr.source_shards_u8(dirs[1], DIM_IN, augment="rrc", flip=True, seed=7, prefetch=True, antialias=True)
        elif kind == "u8_rrc":
            tr.source_shards_u8(dirs[1], DIM_IN, augment="rrc", flip=True, seed=7, prefetch=True)
        else:
            tr.source_shards_u8(dirs[1], DIM_IN, augment="random", flip=True, seed=7, prefetch=True)
        for _ in range(warmup):  # the first load reads the shard
            tr.step()
            assert tr.L.mi_batch_last_status(tr.c_batch) == 0
        tr.L.mi_device_synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tr.step()
        tr.L.mi_device_synchronize()
        dt = (time.perf_counter() - t0) / steps
        assert tr.L.mi_batch_last_status(tr.c_batch) == 0 and tr.check_errors() == 0
        tr.check()
        return N / dt, tr.device_bytes()
    finally:
        tr.close()


def bench_steps(steps, warmup):
    per_shard = N * (steps + warmup + 1)
    root = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    res = {}
    try:
        f32, u8, sizes = build_shards(root, per_shard)
        for dtype in ("f32", "bf16"):
            kinds = ("f32_shards", "u8_shards", "u8_rrc", "u8_rrc_aa")
            r = {k: [] for k in kinds}
            r["synthetic"], dev = time_leg("synthetic", dtype, (f32, u8), per_shard, steps, warmup)
            for _ in range(3):
                for kind in kinds:
                    r[kind].append(time_leg(kind, dtype, (f32, u8), per_shard, steps, warmup)[0])
            spreads = {k: max(r[k]) - min(r[k]) for k in kinds}
            spread = max(spreads["f32_shards"], spreads["u8_shards"])
            best = {k: max(r[k]) for k in kinds}
            res[dtype] = dict(images_per_sec={k: (round(v, 1) if k == "synthetic" else [round(x, 1) for x in v]) for k, v in r.items()},
                              spread_of_repeats=round(spread, 1), spread_by_leg={k: round(v, 1) for k, v in spreads.items()},
                              gap_to_synthetic={k: round(1 - best[k] / r["synthetic"], 4) for k in best},
                              u8_ge_f32_shards=best["u8_shards"] >= best["f32_shards"] - spread,
                              rrc_ge_random=best["u8_rrc"] >= best["u8_shards"] - spreads["u8_shards"], trainer_device_bytes=dev)
            print("%-4s synthetic %.1f img/s, fp32 shards %s, uint8 shards %s, uint8 rrc %s, uint8 rrc antialiased %s (spread of repeats %.1f, of "
                  "the uint8 leg %.1f)" %
                  (dtype, r["synthetic"], ["%.1f" % x for x in r["f32_shards"]], ["%.1f" % x for x in r["u8_shards"]],
                   ["%.1f" % x for x in r["u8_rrc"]], ["%.1f" % x for x in r["u8_rrc_aa"]], spread, spreads["u8_shards"]))
        img_in, img_out = DIM_IN * DIM_IN * 3, DIM_OUT * DIM_OUT * 3 * 4
        res["bytes"] = dict(
            shard_files=sizes, images_per_shard=per_shard,
            reference_shard_32768=dict(f32=32768 * (img_out + 4), u8=32768 * (img_in + 4 + 8)),
            per_step_h2d=dict(f32=N * (img_out + 4), u8=N * (img_in + 4 + 12)),
            pinned_host_with_prefetch=dict(f32=2 * N * (img_out + 4), u8=2 * N * (img_in + 20) + 2 * N * 4 + N * img_out),
            device_beside_the_trainer_with_prefetch=dict(f32=3 * N * img_out + 2 * N * 4, u8=2 * N * (img_out + 4) + 2 * N * (img_in + 20)))
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-steps", action="store_true", help="time the two kernels only")
    a = ap.parse_args()
    if B.load().mi_device_count() < 1:
        raise RuntimeError("bench_input needs a HIP device")
    out = {"kernels": bench_kernels(max(a.runs, 20))}
    out["resample"] = bench_resample(max(a.runs, 20))
    ok = out["kernels"]["decode_le_nhwc"]
    if not a.skip_steps:
        out["steps"] = bench_steps(max(a.steps, 16), a.warmup)
        ok = ok and all(out["steps"][d]["u8_ge_f32_shards"] and out["steps"][d]["rrc_ge_random"] for d in ("f32", "bf16"))
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
