"""Gradient accumulation in numpy float32 (include/resnet_mi.h, "gradient accumulation"): the model of grad_accum_kernel and of a window
of k micro-batches.  Every operation is one IEEE float32 operation rounded on its own -- a sum, then a product, never a fused
multiply-add; values that are not finite propagate as IEEE has them.  tests/test_accum_model.py pins it against torch on the CPU.
"""
import numpy as np

FIRST, ADD, FOLD = 0, 1, 2


def _f32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.float32) if a.dtype == np.uint32 else a.astype(np.float32, copy=False)


def first(g):
    """acc = g: the words of g (NaN payloads and -0 as they are)"""
    return _f32(g).copy()


def add(acc, g):
    """acc = acc (+) g"""
    with np.errstate(all="ignore"):
        return (_f32(acc) + _f32(g)).astype(np.float32)


def fold(acc, g, scale):
    """g = (acc (+) g) (x) scale; float32 times a float32 scalar stays float32 in numpy, one rounding each"""
    with np.errstate(all="ignore"):
        s = (_f32(acc) + _f32(g)).astype(np.float32)
        return (s * np.float32(scale)).astype(np.float32)


def fold_once(acc, g, scale):
    """what the fold must NOT compute: (acc + g) scale evaluated in double and rounded to float32 at the end (what a fused
    multiply-add, or arithmetic kept in a wider type, would give)"""
    with np.errstate(all="ignore"):
        return ((_f32(acc).astype(np.float64) + _f32(g).astype(np.float64)) * np.float64(np.float32(scale))).astype(np.float32)


def separating_pair(n, scale, seed):
    """(acc, g) of n float32, acc ~ N(0, 1) and g ~ 1e-4 N(0, 1), in which EVERY element tells fold from fold_once at this scale, and
    acc != g everywhere: candidates are drawn and the ones the model separates are kept, in the order drawn"""
    rng = np.random.RandomState(seed)
    accs, gs, have = [], [], 0
    while have < n:
        m = 16 * (n - have) + 4096
        acc, g = rng.randn(m).astype(np.float32), (rng.randn(m) * 1e-4).astype(np.float32)
        keep = (fold(acc, g, scale).view(np.uint32) != fold_once(acc, g, scale).view(np.uint32)) & (acc != g)
        accs.append(acc[keep])
        gs.append(g[keep])
        have += int(keep.sum())
    return np.concatenate(accs)[:n].copy(), np.concatenate(gs)[:n].copy()


def window(gs, scale):
    """what the optimizer is handed after a window over the micro-batch gradients gs[0 .. k): first, add ..., and the last one folded in.
    (k = 1 is the product alone; the trainer runs no window at k = 1 and applies no scale)"""
    gs = [_f32(g) for g in gs]
    if len(gs) == 1:
        with np.errstate(all="ignore"):
            return (gs[0] * np.float32(scale)).astype(np.float32)
    acc = first(gs[0])
    for g in gs[1:-1]:
        acc = add(acc, g)
    return fold(acc, gs[-1], scale)


def accumulator(gs):
    """the accumulator after the collecting calls over gs (at least one)"""
    acc = first(gs[0])
    for g in gs[1:]:
        acc = add(acc, g)
    return acc


def same(got, want):
    """bit for bit, except that a NaN matches any NaN: IEEE 754 leaves the sign and payload of a NaN that an operation produces or passes
    on to the implementation (x86 and the GPU differ), and only `first`, which does no arithmetic, promises them"""
    got, want = _f32(got), _f32(want)
    if got.shape != want.shape:
        return False
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
