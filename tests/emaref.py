"""The model of weight averaging (include/resnet_mi.h, "weight averaging"), in numpy.

weight(decay, warmup, k)      the weight of EMA update k in Python doubles, rounded to float32 once
fma32(a, b, c)                an exact float32 fused multiply-add
lerp32(e, p, w)               torch.lerp's float32 bits with the library's rule for results that are not finite
ema_run(params_per_step, ...) a whole run: the counter, `every`, the warm-up

fma32 is exact.  The product of two float32 values is exact in float64 (48 bits).  Its sum with a float32 value is not, and rounding it
to float64 and then to float32 rounds twice.  So the float64 sum is taken with its error term (Knuth's two-sum, error-free) and rounded
to ODD: where the sum is inexact and its last mantissa bit is even, it moves one unit towards the error.  A round-to-odd value of 53 bits
rounds to any narrower format with at most 51 bits (float32's 24, fewer for its subnormals) as the exact value would.
"""
import numpy as np


def weight(decay, warmup, k):
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + float(k)) / (10.0 + float(k)))
    return np.float32(1.0 - d)


def fma32(a, b, c):
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        prod = a * b                       # exact: 24 x 24 bits
        s = prod + c
        bb = s - prod                      # two-sum: s + err == prod + c exactly (where everything is finite)
        err = (prod - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((np.ascontiguousarray(s).view(np.int64) & 1) == 0)
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def lerp32(e, p, w):
    """e' = fmaf(w, p - e, e) for w < 0.5, fmaf(-(1 - w), p - e, p) otherwise; an element whose result is not finite keeps e"""
    e, p = np.asarray(e, np.float32), np.asarray(p, np.float32)
    w = np.float32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p - e).astype(np.float32)
        r = fma32(w, d, e) if w < np.float32(0.5) else fma32(-(np.float32(1.0) - w), d, p)
    return np.where(np.isfinite(r), r, e).astype(np.float32)


def ema_run(params_per_step, start, decay, every=1, warmup=False, counter=0, updates_before=0):
    """start: the list of arrays the EMA holds (the snapshot); params_per_step[s]: the list of arrays the trainer holds after its update
    number updates_before + s + 1.  Returns per step (list of arrays, counter).  every == 0: nothing moves"""
    cur = [np.array(a, np.float32) for a in start]
    out = []
    for s, params in enumerate(params_per_step):
        n_updates = updates_before + s + 1
        if every > 0 and n_updates % every == 0:
            w = weight(decay, warmup, counter)
            cur = [lerp32(c, p, w) for c, p in zip(cur, params)]
            counter += 1
        out.append(([c.copy() for c in cur], counter))
    return out
