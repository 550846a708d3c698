"""numpy / math restatement of random erasing (include/resnet_mi.h, "random erasing"): the plan of mi_erase_plan (Python ints and floats,
math.log / exp / sqrt and round, which rounds half to even as lrint does), the noise of MI_ERASE_NOISE on uint64 arrays, and the in-place
fill of mi_op_erase_batch (kernels_input.hip) in float32."""
import math

import numpy as np

from mixref import M64, splitmix64_at, unit

TRIES = 10
STEP_INDEX = 1000     # e = splitmix64_at(k, 1000): the mix plan draws indices up to 131 from the same step key k
NOISE_OFFSET = 64     # g_m = splitmix64_at(q, 64 + 3 el + m)
NOISE_MEAN = 393210   # 12 fields x 65535 / 2
_G = np.uint64(0x9E3779B97F4A7C15)


def step_key(seed, epoch, step, rank, world):
    """e: the key of one step's rows, and the noise seed the trainer passes"""
    s = splitmix64_at(seed & M64, epoch)
    k = splitmix64_at(s, step * world + rank)
    return splitmix64_at(k, STEP_INDEX)


def plan_rows(seed, epoch, step, rank, world, n, dim, prob, scale, ratio):
    """(boxes, drawn, taken): boxes int32 (n, 4) rows (y0, x0, h, w), all 0 without a box; drawn[i]: U(d(0)) < prob; taken[i]: one of the
    ten tries gave h < D and w < D (its box may still be empty at tiny D)"""
    e = step_key(seed, epoch, step, rank, world)
    D = dim
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    boxes = np.zeros((n, 4), np.int32)
    drawn, taken = np.zeros(n, bool), np.zeros(n, bool)
    for i in range(n):
        k = splitmix64_at(e, i)
        if unit(splitmix64_at(k, 0)) >= prob:
            continue
        drawn[i] = True
        for t in range(TRIES):
            target = (float(D) * float(D)) * (scale[0] + unit(splitmix64_at(k, 1 + 4 * t)) * (scale[1] - scale[0]))
            r = math.exp(log_lo + unit(splitmix64_at(k, 2 + 4 * t)) * (log_hi - log_lo))
            fh, fw = math.sqrt(target * r), math.sqrt(target / r)
            if not (fh < D + 1.0 and fw < D + 1.0):  # rounds to D or more: not taken (and round() of an infinity raises)
                continue
            h, w = round(fh), round(fw)
            if not (h < D and w < D):
                continue
            y0 = ((splitmix64_at(k, 3 + 4 * t) >> 32) * (D - h + 1)) >> 32
            x0 = ((splitmix64_at(k, 4 + 4 * t) >> 32) * (D - w + 1)) >> 32
            boxes[i] = (y0, x0, h, w)
            taken[i] = True
            break
    return boxes, drawn, taken


def plan(seed, epoch, step, rank, world, n, dim, prob, scale=(0.02, 0.33), ratio=(0.3, 3.3)):
    return plan_rows(seed, epoch, step, rank, world, n, dim, prob, scale, ratio)[0]


def clamp_box(y0, x0, h, w, D):
    """the box as launcher and kernel clamp it: y0 into [0, D], h into [0, D - y0], x likewise"""
    y0 = min(max(int(y0), 0), D)
    x0 = min(max(int(x0), 0), D)
    return y0, x0, min(max(int(h), 0), D - y0), min(max(int(w), 0), D - x0)


def _splitmix_np(seed, i):
    """splitmix64_at on a uint64 array of indices (arithmetic modulo 2^64)"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (i + np.uint64(1)) * _G
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def noise_at(noise_seed, row, el):
    """z (float32) of batch row `row` (its noise key index) at the element positions el = (c D + y) D + x, any integer array"""
    q = splitmix64_at(noise_seed & M64, row)
    el = np.asarray(el).astype(np.uint64)
    S = np.zeros(el.shape, np.int64)
    for m in range(3):
        g = _splitmix_np(q, np.uint64(NOISE_OFFSET) + np.uint64(3) * el + np.uint64(m))
        for f in range(4):
            S += ((g >> np.uint64(16 * f)) & np.uint64(0xFFFF)).astype(np.int64)
    return (S - NOISE_MEAN).astype(np.float32) * np.float32(2.0 ** -16)  # both steps exact: |S - mean| < 2^20


def noise(noise_seed, row, D):
    """z of every element of a (3, D, D) image"""
    return noise_at(noise_seed, row, np.arange(3 * D * D, dtype=np.uint64)).reshape(3, D, D)


def erase(images, boxes, mode="const", value=(0, 0, 0), std=(1, 1, 1), noise_seed=0, first_row=0):
    """the batch (n, 3, D, D) float32 with row i's box (y0, x0, h, w) filled: plane c with value[c], or with value[c] (+) std[c] (x) z, the
    product and the sum float32 operations of their own.  Everything outside the boxes keeps its bits"""
    x = np.array(images, np.float32, copy=True)
    n, D = x.shape[0], x.shape[2]
    value, std = np.asarray(value, np.float32), np.asarray(std, np.float32)
    for i in range(n):
        y0, x0, h, w = clamp_box(*boxes[i], D)
        if h == 0 or w == 0:
            continue
        if mode == "const":
            for c in range(3):
                x[i, c, y0:y0 + h, x0:x0 + w] = value[c]
        else:
            yy, xx = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
            for c in range(3):
                z = noise_at(noise_seed, first_row + i, (c * D + yy) * D + xx)
                x[i, c, y0:y0 + h, x0:x0 + w] = value[c] + std[c] * z
    return x
