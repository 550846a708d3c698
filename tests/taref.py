"""numpy / math restatement of TrivialAugmentWide (include/resnet_mi.h, "TrivialAugmentWide"): the per-row record of mi_ta_row (Python
floats and math.atan / tan / cos / sin / radians / degrees / round, as torchvision and Pillow compute it), the plan of mi_ta_plan, and the
fourteen Pillow operations on uint8 planes (3, D, D) = (R, G, B) in numpy int / float32 / float64 with every operation rounded on its
own.  apply_batch is mi_op_trivial_augment: decode o Pillow-op o quantise on the fp32 batch, identity rows untouched."""
import math

import numpy as np

from mixref import M64, splitmix64_at

OPS = ["Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness", "Posterize",
       "Solarize", "AutoContrast", "Equalize"]
(IDENTITY, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE, SOLARIZE, AUTOCONTRAST,
 EQUALIZE) = range(14)
N_OPS, N_BINS = 14, 31
SIGNED = (SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS)
GEOMETRIC = (SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE)
STEP_INDEX = 2000  # a = splitmix64_at(k, 2000): the mix plan draws indices up to 131 from the step key k, the erase plan index 1000

# torch.linspace(0, 0.99, 31) and torch.linspace(0, 32, 31) in float32, widened to double (test_ta_model compares with torch on the spot)
MAG_099 = [0.0, 0.032999999821186066, 0.06599999964237213, 0.0989999994635582, 0.13199999928474426, 0.16499999165534973,
           0.1979999989271164, 0.23100000619888306, 0.2639999985694885, 0.296999990940094, 0.32999998331069946, 0.3630000054836273,
           0.3959999978542328, 0.42899999022483826, 0.4620000123977661, 0.4950000047683716, 0.527999997138977, 0.5609999895095825,
           0.593999981880188, 0.6270000338554382, 0.6600000262260437, 0.6930000185966492, 0.7260000109672546, 0.7590000033378601,
           0.7919999957084656, 0.824999988079071, 0.8580000400543213, 0.8910000324249268, 0.9240000247955322, 0.9570000171661377,
           0.9900000095367432]
MAG_32 = [0.0, 1.0666667222976685, 2.133333444595337, 3.200000286102295, 4.266666889190674, 5.333333492279053, 6.40000057220459,
          7.466667175292969, 8.533333778381348, 9.600000381469727, 10.666666984558105, 11.733333587646484, 12.80000114440918,
          13.866667747497559, 14.933334350585938, 15.999999046325684, 17.066665649414062, 18.133333206176758, 19.19999885559082,
          20.266666412353516, 21.333332061767578, 22.399999618530273, 23.46666717529297, 24.53333282470703, 25.600000381469727,
          26.66666603088379, 27.733333587646484, 28.799999237060547, 29.866666793823242, 30.933332443237305, 32.0]

MEAN_OF_SRC = (123.68, 116.78, 103.94)  # g_decode_table: subtracted from source position p; plane d holds position 2 - d
F32 = np.float32


def mean_plane(d):
    return F32(MEAN_OF_SRC[2 - d])


def decode(b):
    """uint8 (..., 3, D, D) -> float32: g_decode_table's value, one rounding made from a double"""
    b = np.asarray(b)
    m = np.array([MEAN_OF_SRC[2 - d] for d in range(3)], np.float64).reshape(3, 1, 1)
    return (b.astype(F32).astype(np.float64) - m).astype(F32)


def quantise(v):
    """float32 (..., 3, D, D) -> uint8: one fp32 addition of the plane's mean, NaN -> 0, clamp to [0, 255], round half to even"""
    v = np.asarray(v, F32)
    m = np.array([mean_plane(d) for d in range(3)], F32).reshape(3, 1, 1)
    with np.errstate(invalid="ignore"):
        s = v + m
        s = np.where(np.isnan(s), F32(0), np.minimum(np.maximum(s, F32(0)), F32(255)))
    return np.rint(s).astype(np.uint8)


# ---- the record ----
def magnitude(op, bin):
    if op in (SHEAR_X, SHEAR_Y, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS):
        return MAG_099[bin]
    if op in (TRANSLATE_X, TRANSLATE_Y):
        return MAG_32[bin]
    if op == ROTATE:
        return 4.5 * bin
    if op == POSTERIZE:
        return float(8 - round(bin / 5))
    if op == SOLARIZE:
        return 255.0 - 8.5 * bin
    return 0.0


def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def matrix(op, m, D):
    """the inverse affine matrix (a0 .. a5) torchvision hands to Pillow for a PIL image"""
    if op in (SHEAR_X, SHEAR_Y):
        t = math.tan(math.radians(math.degrees(math.atan(m))))
        return (1.0, t, 0.0, 0.0, 1.0, 0.0) if op == SHEAR_X else (1.0, 0.0, 0.0, t, 1.0, 0.0)
    if op == TRANSLATE_X:
        return (1.0, 0.0, float(-int(m)), 0.0, 1.0, 0.0)
    if op == TRANSLATE_Y:
        return (1.0, 0.0, 0.0, 0.0, 1.0, float(-int(m)))
    assert op == ROTATE
    r = -math.radians(m % 360.0)
    a0, a1, a3, a4 = round(math.cos(r), 15), round(math.sin(r), 15), round(-math.sin(r), 15), round(math.cos(r), 15)
    c = D / 2.0
    a2 = a0 * -c + a1 * -c + 0.0
    a5 = a3 * -c + a4 * -c + 0.0
    return (a0, a1, a2 + c, a3, a4, a5 + c)


def fixed(a):
    """Pillow's 16.16 coefficients, the half-pixel offset folded into A2 and A5"""
    return [fix(a[0]), fix(a[1]), fix(a[2] + a[0] * 0.5 + a[1] * 0.5), fix(a[3]), fix(a[4]), fix(a[5] + a[3] * 0.5 + a[4] * 0.5)]


def row(op, bin, neg, D):
    """mi_ta_row: dict(op, bin, neg, magnitude, factor, arg, A)"""
    assert 0 <= op < N_OPS and 0 <= bin < N_BINS and neg in (0, 1) and 1 <= D <= 4096
    neg = neg if op in SIGNED else 0
    m = magnitude(op, bin)
    if neg:
        m = -m
    r = dict(op=op, bin=bin, neg=neg, magnitude=m, factor=F32(0), arg=0, A=[0] * 6)
    if op in (BRIGHTNESS, COLOR, CONTRAST, SHARPNESS):
        r["factor"] = F32(1.0 + m)
    elif op == POSTERIZE:
        r["arg"] = ~(2 ** (8 - int(m)) - 1) & 255
    elif op == SOLARIZE:
        r["arg"] = int(math.ceil(m))
    elif op in GEOMETRIC:
        r["A"] = fixed(matrix(op, m, D))
    return r


def plan(seed, epoch, step, rank, world, n, D):
    """mi_ta_plan: the rows of one step"""
    s = splitmix64_at(seed & M64, epoch)
    k = splitmix64_at(s, step * world + rank)
    a = splitmix64_at(k, STEP_INDEX)
    rows = []
    for i in range(n):
        ki = splitmix64_at(a, i)
        op = ((splitmix64_at(ki, 0) >> 32) * N_OPS) >> 32
        bin = ((splitmix64_at(ki, 1) >> 32) * N_BINS) >> 32
        neg = splitmix64_at(ki, 2) >> 63
        rows.append(row(int(op), int(bin), int(neg), D))
    return rows


# ---- the operations on uint8 (3, D, D) ----
def blend(d, x, f):
    """Pillow's ImagingBlend on bytes: d (+) f (x) (x (-) d) in float32; inside [0, 1] truncated, outside clipped then truncated"""
    f = F32(f)
    d, x = np.asarray(d).astype(F32), np.asarray(x).astype(F32)
    t = d + f * (x - d)
    if 0 <= f <= 1:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def luma(img):
    r, g, b = (img[c].astype(np.int64) for c in range(3))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def color(img, f):
    return blend(np.broadcast_to(luma(img), img.shape), img, f)


def contrast_mean(img):
    D2 = img.shape[1] * img.shape[2]
    return (2 * int(luma(img).astype(np.int64).sum()) + D2) // (2 * D2)


def contrast(img, f):
    return blend(np.full_like(img, contrast_mean(img)), img, f)


def smooth(img):
    """ImageFilter.SMOOTH: (1 1 1; 1 5 1; 1 1 1) / 13 in float32 from 0.5, products added in row-major order; the border is the source"""
    _, H, W = img.shape
    out = img.copy()
    if H < 3 or W < 3:
        return out
    k = [F32(1.0 / 13)] * 9
    k[4] = F32(5.0 / 13)
    x = img.astype(F32)
    acc = np.full((3, H - 2, W - 2), F32(0.5))
    for dy in range(3):
        for dx in range(3):
            acc = acc + x[:, dy:dy + H - 2, dx:dx + W - 2] * k[3 * dy + dx]
    out[:, 1:H - 1, 1:W - 1] = np.where(acc <= 0, 0, np.where(acc >= 255, 255, acc.astype(np.int32))).astype(np.uint8)
    return out


def sharpness(img, f):
    return blend(smooth(img), img, f)


def posterize(img, mask):
    return img & np.uint8(mask)


def solarize(img, bound):
    return np.where(img < bound, img, 255 - img).astype(np.uint8)


def autocontrast_lut(h):
    """one channel's table from its histogram"""
    occ = np.flatnonzero(h)
    i = np.arange(256)
    if len(occ) == 0 or occ[-1] <= occ[0]:
        return i.astype(np.uint8)
    lo, hi = int(occ[0]), int(occ[-1])
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    v = (i.astype(np.float64) * scale + off).astype(np.int64)  # product, then sum; truncation toward zero
    return np.clip(v, 0, 255).astype(np.uint8)


def equalize_lut(h):
    occ = np.flatnonzero(h)
    ident = np.arange(256).astype(np.uint8)
    if len(occ) < 2:
        return ident
    step = (int(h.sum()) - int(h[occ[-1]])) // 255
    if step == 0:
        return ident
    n = step // 2 + np.concatenate([[0], np.cumsum(h.astype(np.int64))[:-1]])
    return np.minimum(255, n // step).astype(np.uint8)


def _per_channel(img, make):
    out = np.empty_like(img)
    for c in range(3):
        out[c] = make(np.bincount(img[c].ravel(), minlength=256))[img[c]]
    return out


def autocontrast(img):
    return _per_channel(img, autocontrast_lut)


def equalize(img):
    return _per_channel(img, equalize_lut)


def affine(img, A):
    """Pillow's nearest affine in 16.16 fixed point; outside the source: 0"""
    _, H, W = img.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    xin = (A[2] + A[1] * y + A[0] * x) >> 16
    yin = (A[5] + A[4] * y + A[3] * x) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    src = img[:, np.where(ok, yin, 0), np.where(ok, xin, 0)]
    return np.where(ok, src, 0).astype(np.uint8)


def apply(img, r):
    """one uint8 image (3, D, D) under the record r"""
    op = r["op"]
    if op == IDENTITY:
        return img.copy()
    if op in GEOMETRIC:
        return affine(img, r["A"])
    if op == BRIGHTNESS:
        return brightness(img, r["factor"])
    if op == COLOR:
        return color(img, r["factor"])
    if op == CONTRAST:
        return contrast(img, r["factor"])
    if op == SHARPNESS:
        return sharpness(img, r["factor"])
    if op == POSTERIZE:
        return posterize(img, r["arg"])
    if op == SOLARIZE:
        return solarize(img, r["arg"])
    if op == AUTOCONTRAST:
        return autocontrast(img)
    assert op == EQUALIZE
    return equalize(img)


def apply_batch(x, rows):
    """mi_op_trivial_augment: float32 (n, 3, D, D); identity rows keep their bits"""
    out = np.array(x, F32, copy=True)
    for i, r in enumerate(rows):
        if r["op"] != IDENTITY:
            out[i] = decode(apply(quantise(x[i]), r))
    return out
