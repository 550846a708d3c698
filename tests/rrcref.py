"""numpy / math restatement of the random-resized crop (include/resnet_mi.h, "random-resized crop"): the box draw of
mi_augment_plan_rrc (torchvision's RandomResizedCrop.get_params on a square image, driven by the splitmix64 counter streams) and the
integer bilinear resample of mi_op_resample_u8 / kernels_input.hip.  Python ints and int64 throughout: nothing here can overflow."""
import math

import numpy as np

import augref
import synth

SCALE, RATIO = (0.08, 1.0), (3 / 4, 4 / 3)
M64 = 0xFFFFFFFFFFFFFFFF


def unit(x):
    """U(x) = (x >> 11) 2^-53"""
    return float(int(x) >> 11) * 2.0 ** -53


def box(d, flip, dim_in, scale, ratio):
    """(row0, col0, h, w, flip) from the image's draws d(0 .. 40) (Python ints)"""
    area = float(dim_in) * float(dim_in)
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    fl = (d[40] >> 63) if flip else 0
    for t in range(10):
        target = area * (scale[0] + unit(d[4 * t]) * (scale[1] - scale[0]))
        r = math.exp(log_lo + unit(d[4 * t + 1]) * (log_hi - log_lo))
        fw, fh = math.sqrt(target * r), math.sqrt(target / r)
        if not (fw <= dim_in + 1 and fh <= dim_in + 1):  # round() of an infinity raises; such a side is refused below anyway
            continue
        w, h = round(fw), round(fh)  # half to even, as lrint
        if 1 <= w <= dim_in and 1 <= h <= dim_in:
            row0 = ((d[4 * t + 2] >> 32) * (dim_in - h + 1)) >> 32
            col0 = ((d[4 * t + 3] >> 32) * (dim_in - w + 1)) >> 32
            return row0, col0, h, w, fl
    h = w = dim_in
    if ratio[0] > 1:
        h = min(max(round(dim_in / ratio[0]), 1), dim_in)
    elif ratio[1] < 1:
        w = min(max(round(dim_in * ratio[1]), 1), dim_in)
    return (dim_in - h) // 2, (dim_in - w) // 2, h, w, fl


def plan(flip, seed, epoch, first_global_index, n, dim_in, scale=SCALE, ratio=RATIO):
    """int32 (n, 5): row0, col0, box_h, box_w, flip of the images with global indices first_global_index .. + n"""
    s = augref.splitmix64_at(seed & M64, epoch)
    keys = synth.splitmix64(s, n, offset=int(first_global_index))
    draws = np.stack([synth.splitmix64(k, 41) for k in keys]) if n else np.zeros((0, 41), np.uint64)  # d(j) = splitmix64_at(k, j)
    return np.array([box(d, flip, dim_in, scale, ratio) for d in draws.tolist()], np.int32).reshape(n, 5)


def clamp_box(b, dim_in):
    """the box as the kernel clamps it: h, w -> [1, dim_in], row0 -> [0, dim_in - h], col0 -> [0, dim_in - w]"""
    r0, c0, h, w, fl = (int(v) for v in b)
    h, w = min(max(h, 1), dim_in), min(max(w, 1), dim_in)
    return min(max(r0, 0), dim_in - h), min(max(c0, 0), dim_in - w), h, w, int(fl != 0)


def coords(length, D, flip=False):
    """(i0, i1, weight of i1 in 1/256) per output index of an axis that scales `length` source pixels to D"""
    o = np.arange(D, dtype=np.int64)
    if flip:
        o = D - 1 - o
    num = np.clip((2 * o + 1) * length - D, 0, (length - 1) * 2 * D)
    f = (num * 256) // (2 * D)
    i0 = f >> 8
    return i0, np.minimum(i0 + 1, length - 1), f & 255


def resample(src, boxes, dim_out):
    """src uint8 (n, dim_in, dim_in, 3) B,G,R; boxes (n, 5) -> float32 (n, 3, dim_out, dim_out), planes R,G,B"""
    n, dim_in = src.shape[0], src.shape[1]
    out = np.empty((n, 3, dim_out, dim_out), np.float32)
    for i in range(n):
        r0, c0, h, w, fl = clamp_box(boxes[i], dim_in)
        b = src[i, r0:r0 + h, c0:c0 + w, :].astype(np.int64)
        y0, y1, wy = coords(h, dim_out)
        x0, x1, wx = coords(w, dim_out, fl)
        wy, wx = wy[:, None, None], wx[None, :, None]
        top = b[y0][:, x0] * (256 - wx) + b[y0][:, x1] * wx
        bot = b[y1][:, x0] * (256 - wx) + b[y1][:, x1] * wx
        v = top * (256 - wy) + bot * wy
        assert v.max() <= 255 * 65536
        for d in range(3):
            out[i, d] = (v[:, :, 2 - d].astype(np.float64) * 2.0 ** -16 - augref.MEAN_OF_SRC[2 - d]).astype(np.float32)
    return out


RS_ROWS, RS_LDS_MAX = 16, 65536


def src_rows(rows, dim_in, dim_out):
    return -(-(rows - 1) * dim_in // dim_out) + 2


def lds_bytes(rows, dim_in, dim_out):
    """the launcher's LDS need with `rows` output rows per workgroup (include/resnet_mi.h, mi_op_resample_u8)"""
    up4 = lambda v: (v + 3) & ~3
    return 4 * (up4(dim_out) + up4(rows)) + src_rows(rows, dim_in, dim_out) * 16 * ((3 * dim_in + 30) // 16)


def launch_rows(dim_in, dim_out):
    """output rows per workgroup the launcher picks, 0: not even one fits (-2)"""
    for rows in range(min(RS_ROWS, dim_out), 0, -1):
        if lds_bytes(rows, dim_in, dim_out) <= RS_LDS_MAX:
            return rows
    return 0
