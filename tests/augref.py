"""numpy restatement of the uint8 input path (include/resnet_mi.h, "uint8 shards"): the augmentation plan rule of mi_augment_plan and
the decode of mi_op_decode_u8 / kernels_input.hip (crop, flip, B,G,R -> R,G,B planes, mean subtraction through the 3 x 256 table).
The decode of a FIXED plan is build_training_shards.c:88-144, i.e. what tests/golden/shard_ref_golden.npz (written by the reference
binary) holds."""
import numpy as np

import synth

FIXED, CENTER, RANDOM = 0, 1, 2
MEAN_OF_SRC = (123.68, 116.78, 103.94)  # subtracted from source byte 0 (B), 1 (G), 2 (R)


def table():
    """[3][256] float32: (float)((double)(float)byte - mean), one rounding made from a double"""
    b = np.arange(256, dtype=np.float32).astype(np.float64)
    return np.stack([(b - m).astype(np.float32) for m in MEAN_OF_SRC])


def splitmix64_at(seed, i):
    """element i of the counter stream `seed` (synth.splitmix64 numbers its elements from offset + 1)"""
    return synth.splitmix64(seed, 1, offset=int(i))[0]


def plan(mode, flip, seed, epoch, first_global_index, n, dim_in, dim_out, fixed_crops=None):
    """int32 (n, 3): row_off, col_off, flip of the images with global indices first_global_index .. + n"""
    R = dim_in - dim_out
    out = np.zeros((n, 3), np.int32)
    if mode == FIXED:
        out[:, :2] = np.asarray(fixed_crops, np.int32).reshape(n, 2)
    elif mode == CENTER:
        out[:, :2] = R // 2
    else:
        s = splitmix64_at(seed & 0xFFFFFFFFFFFFFFFF, epoch)
        r = synth.splitmix64(s, n, offset=int(first_global_index))
        m = np.uint64(0xFFFFF)
        out[:, 0] = ((r & m) * np.uint64(R + 1)) >> np.uint64(20)
        out[:, 1] = (((r >> np.uint64(20)) & m) * np.uint64(R + 1)) >> np.uint64(20)
        if flip:
            out[:, 2] = r >> np.uint64(63)
    return out


def decode(src, pl, dim_out):
    """src uint8 (n, dim_in, dim_in, 3) B,G,R; pl (n, 3) -> float32 (n, 3, dim_out, dim_out), planes R,G,B"""
    t = table()
    n = src.shape[0]
    out = np.empty((n, 3, dim_out, dim_out), np.float32)
    for i in range(n):
        ro, co, fl = (int(v) for v in pl[i])
        crop = src[i, ro:ro + dim_out, co:co + dim_out, :]
        if fl:
            crop = crop[:, ::-1, :]
        for d in range(3):
            out[i, d] = t[2 - d][crop[:, :, 2 - d]]
    return out
