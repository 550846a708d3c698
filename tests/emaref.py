"""The model of weight averaging (include/resnet_mi.h, "weight averaging"), in numpy.

weight(decay, warmup, k)      the weight of EMA update k in Python doubles, rounded to float32 once
fma32(a, b, c)                an exact float32 fused multiply-add
lerp32(e, p, w)               torch.lerp's float32 bits with the library's rule for results that are not finite
unfused32, other_branch32     the two slightly wrong kernels; alternative32(e, p, w) is the one the weight w is there to catch
separating_pair(n, w, seed)   inputs in which every element tells lerp32 from alternative32
tail_and_partial_turn(...)    the positions the streaming kernels handle outside a whole unrolled turn
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


def unfused32(e, p, w):
    """what the kernel must NOT compute: the same branch with the product and the sum rounded one after the other"""
    e, p = np.asarray(e, np.float32), np.asarray(p, np.float32)
    w = np.float32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p - e).astype(np.float32)
        r = (e + (w * d).astype(np.float32)) if w < np.float32(0.5) else (p + (-(np.float32(1.0) - w) * d).astype(np.float32))
        r = r.astype(np.float32)
    return np.where(np.isfinite(r), r, e).astype(np.float32)


def other_branch32(e, p, w):
    """the fused branch that w does NOT select (w < 0.5 read as w >= 0.5 and the other way round)"""
    e, p = np.asarray(e, np.float32), np.asarray(p, np.float32)
    w = np.float32(w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (p - e).astype(np.float32)
        r = fma32(-(np.float32(1.0) - w), d, p) if w < np.float32(0.5) else fma32(w, d, e)
    return np.where(np.isfinite(r), r, e).astype(np.float32)


def alternative32(e, p, w):
    """the wrong kernel a weight is there to catch: the other branch at w = 0.5 (the comparison written <=), the unfused update elsewhere"""
    return other_branch32(e, p, w) if np.float32(w) == np.float32(0.5) else unfused32(e, p, w)


def separating_pair(n, w, seed):
    """(e, p) of n float32 in the distribution of the operator tests (e ~ 0.1 N(0, 1), p - e ~ 0.01 N(0, 1)) in which EVERY element tells
    lerp32 from alternative32 at the weight w: candidates are drawn and the ones the model separates are kept, in the order drawn"""
    rng = np.random.RandomState(seed)
    es, ps, have = [], [], 0
    while have < n:
        m = 64 * (n - have) + 4096
        e = (0.1 * rng.randn(m)).astype(np.float32)
        p = (e + 0.01 * rng.randn(m)).astype(np.float32)
        keep = lerp32(e, p, w).view(np.uint32) != alternative32(e, p, w).view(np.uint32)
        es.append(e[keep])
        ps.append(p[keep])
        have += int(keep.sum())
    return np.concatenate(es)[:n].copy(), np.concatenate(ps)[:n].copy()


def tail_and_partial_turn(n, turn_floats, vector):
    """the positions of an arena of n floats that the streaming kernels (ema_update, exchange, grad_accum) do not handle in a whole unrolled
    turn: the floats of the last, partial turn (turn_floats per workgroup turn in this instantiation) and, in the vector instantiation, the
    n % 4 floats behind the last 16-byte group"""
    at = np.zeros(n, bool)
    body = n - n % 4 if vector else n
    at[body // turn_floats * turn_floats:] = True
    return at


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
