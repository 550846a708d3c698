"""Per-step training-loss curves of the CPU models of the reference-defined ResNet-50 (CPU only; no GPU, no product code).

The benchmark's setting: the bench's own init (synth.make_params(R50_DIMS), undamped), lr 1e-4, Adam (0.9, 0.999, eps 1e-7),
the two-batch synthetic pool (step s trains on synth.make_batch(step=s % 2)), here at batch 8.  Four executions, each with
the float64 numpy Adam of tests/torch_ref.py (decays advance before use) on its own trajectory:

  f64       TorchNet, float64 arithmetic, fp32-free: the exact curve the fp32 product must track
  bf16_f64  TorchNetBF16, float64 arithmetic with bf16 rounding at the product's storage points and batch-norm statistics
            taken before the rounding (the product's rule), its own ReLU gates
  bf16_f32  the same rounding rule with float32 arithmetic: a second valid execution of bf16 storage
  f32       TorchNet with float32 arithmetic: a valid fp32 execution, other summation order than the product's

The spread between the two bf16 executions is what bf16 storage ALONE leaves undetermined, and the spread between f32 and f64
what fp32 arithmetic leaves undetermined; tests/test_gpu_trajectory.py derives its bands from them.  Writes tests/golden/trajectory_r50_b8.npz (loss per image, per step):

  python tools/trajectory_curves.py [--batch 8] [--steps 25] [--out tests/golden/trajectory_r50_b8.npz]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import synth  # noqa: E402
import torch_ref  # noqa: E402

HYPER = dict(lr=1e-4, wd=0.0, b1=0.9, b2=0.999, eps=1e-7)
KINDS = ("f64", "bf16_f64", "bf16_f32", "f32")
THREADS = 4  # float32 sums depend on the thread count: a fixed one makes the float32 curves reproducible


def curve(kind, batch, steps, dims=synth.R50_DIMS, log=None):
    """per-image loss of each of `steps` training steps of one execution `kind` (KINDS)"""
    import torch
    torch.set_num_threads(THREADS)
    params = [p.astype(np.float64) for p in synth.make_params(dims)]
    means = [np.zeros_like(p) for p in params]
    vars_ = [np.zeros_like(p) for p in params]
    out = []
    for s in range(steps):
        im, lab = synth.make_batch(dims, batch, step=s % 2)
        if kind in ("f64", "f32"):
            net = torch_ref.TorchNet(dims, params, eps=HYPER["eps"], dtype=torch.float64 if kind == "f64" else torch.float32)
        else:  # the matrix-core stem of 224x224 inputs stores its own output as bf16 too
            net = torch_ref.TorchNetBF16(dims, params, eps=HYPER["eps"], stem_bf16=True, stats_before_rounding=True,
                                         dtype=torch.float64 if kind == "bf16_f64" else torch.float32)
        loss = float(net.forward(torch_ref.nhwc_to_nchw(im), lab).detach())
        grads = net.backward()
        del net
        t = s + 1
        for i in range(len(params)):
            params[i], means[i], vars_[i] = torch_ref.adam(params[i], grads[i].reshape(params[i].shape), means[i], vars_[i],
                                                           HYPER["b1"] ** t, HYPER["b2"] ** t, **HYPER)
        out.append(loss / batch)
        if log:
            log("%-8s step %2d  loss/image %.6f" % (kind, s, loss / batch))
    return np.array(out, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "trajectory_r50_b8.npz"))
    a = ap.parse_args()
    t0 = time.time()
    res = {k: curve(k, a.batch, a.steps, log=lambda m: print(m, flush=True)) for k in KINDS}
    np.savez(a.out, batch=a.batch, steps=a.steps, **res)
    print("wrote %s in %.0f s" % (a.out, time.time() - t0))
    for s in range(a.steps):
        print("step %2d  " % s + "  ".join("%s %.6f" % (k, res[k][s]) for k in KINDS))


if __name__ == "__main__":
    main()
