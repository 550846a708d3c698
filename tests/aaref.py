"""numpy restatement of the antialiased resize (include/resnet_mi.h, "antialiased resize"): Pillow's Image.resize(size, BILINEAR) on
8-bit images -- the tap tables in float64, every operation rounded on its own, and the two fixed-point passes -- and the launcher's LDS
arithmetic of mi_op_resample_aa_u8.  tests/test_input_aa.py holds it against Pillow itself and against tests/golden/aa_golden.npz."""
import numpy as np

import augref
import rrcref

BITS = 22


def taps(length, V, o):
    """(xmin, K int64 array) of output index o on an axis that scales `length` source pixels to V"""
    scale = float(length) / float(V)
    fs = max(scale, 1.0)
    support, ss = fs, 1.0 / fs
    center = (o + 0.5) * scale
    xmin = max(int(center - support + 0.5), 0)  # int() truncates toward zero, as the C cast
    xmax = min(int(center + support + 0.5), length)
    a = np.abs((np.arange(xmax - xmin) + xmin - center + 0.5) * ss)
    w = np.where(a < 1.0, 1.0 - a, 0.0)
    ww = np.cumsum(w)[-1]  # in order of j: np.sum adds pairwise
    return xmin, (0.5 + w / ww * 4194304.0).astype(np.int64)  # positive: the cast truncates as C's


def table(length, V):
    """the axis as a (V, length) int64 matrix of coefficients"""
    m = np.zeros((V, length), np.int64)
    for o in range(V):
        xmin, K = taps(length, V, o)
        m[o, xmin:xmin + len(K)] = K
    return m


def resize_axis0(img, V):
    """uint8 (length, ...) -> uint8 (V, ...): one pass along axis 0; length == V: skipped"""
    if img.shape[0] == V:
        return img
    acc = np.tensordot(table(img.shape[0], V), img.astype(np.int64), axes=(1, 0)) + (1 << (BITS - 1))
    assert acc.max() < 2 ** 31
    return np.clip(acc >> BITS, 0, 255).astype(np.uint8)


def resize(img, V):
    """uint8 (h, w, c) -> uint8 (V, V, c): the horizontal pass, rounded to bytes, then the vertical one"""
    tmp = resize_axis0(img.transpose(1, 0, 2), V).transpose(1, 0, 2)
    return resize_axis0(tmp, V)


def resample(src, boxes, dim_out, virt=None, win=(0, 0)):
    """src uint8 (n, dim_in, dim_in, 3) B,G,R; boxes (n, 5), clamped as the kernel clamps them -> float32 (n, 3, dim_out, dim_out),
    planes R,G,B: every box scaled to virt^2, the window of dim_out rows and columns at win, flipped within the window"""
    n, dim_in = src.shape[0], src.shape[1]
    virt = dim_out if virt is None else virt
    wr, wc = (win, win) if np.isscalar(win) else win
    out = np.empty((n, 3, dim_out, dim_out), np.float32)
    for i in range(n):
        r0, c0, h, w, fl = rrcref.clamp_box(boxes[i], dim_in)
        b = resize(src[i, r0:r0 + h, c0:c0 + w, :], virt)[wr:wr + dim_out, wc:wc + dim_out, :]
        assert b.shape == (dim_out, dim_out, 3)
        if fl:
            b = b[:, ::-1, :]
        for d in range(3):
            out[i, d] = (b[:, :, 2 - d].astype(np.float32).astype(np.float64) - augref.MEAN_OF_SRC[2 - d]).astype(np.float32)
    return out


# ---- the launcher (kernels_input.hip, mid_resample_aa_u8)
AA_ROWS, AA_LDS_MAX = 16, 65536


def ksize(length, V):
    return 2 * max(-(-length // V), 1) + 1


def src_rows(rows, length, V):
    s = -(-(rows + 1) * length // V) + 1 if length >= V else -(-(rows - 1) * length // V) + 3
    return min(s, length)


def lds_bytes(rows, dim_in, dim_out, virt):
    tables = (4 * (dim_out + rows) * (ksize(dim_in, virt) + 2) + 15) & ~15
    return tables + src_rows(rows, dim_in, virt) * (16 * ((3 * dim_in + 30) // 16) + ((3 * dim_out + 3) & ~3))


def launch_rows(dim_in, dim_out, virt):
    """window rows per workgroup the launcher picks, 0: not even one fits (-2)"""
    for rows in range(min(AA_ROWS, dim_out), 0, -1):
        if lds_bytes(rows, dim_in, dim_out, virt) <= AA_LDS_MAX:
            return rows
    return 0
