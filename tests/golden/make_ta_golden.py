"""Writes tests/golden/ta_golden.npz from Pillow: what the fourteen operations of TrivialAugmentWide give on seeded uint8 images, as
torchvision calls Pillow for a PIL image (Image.transform(AFFINE, NEAREST), Image.rotate, ImageEnhance, ImageOps).  A CRC-32 of the
output per (D, kind, op, bin, sign) at D = 30 and 33 and a dozen outputs in full.  The fixture pins tests/taref.py where Pillow is not
installed.  python tests/golden/make_ta_golden.py"""
import math
import os
import zlib

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
DIMS = (30, 33)
KINDS = ("random", "mixed")
SEED = 20261021
FULL = [(30, "random", 1, 30, 0), (33, "random", 2, 17, 1), (30, "mixed", 3, 30, 1), (33, "mixed", 4, 12, 0), (33, "random", 5, 7, 1),
        (30, "random", 5, 20, 0), (33, "mixed", 6, 30, 0), (30, "random", 7, 25, 1), (33, "mixed", 8, 30, 0), (30, "random", 9, 30, 0),
        (33, "random", 12, 0, 0), (30, "mixed", 13, 0, 0), (33, "random", 13, 0, 0)]  # (D, kind, op, bin, neg)


def image(D, kind):
    """uint8 (3, D, D), planes R, G, B.  random: every byte value, 0 and 255 among them; mixed: R random, G confined to 40 .. 125,
    B constant"""
    rng = np.random.RandomState(SEED + 1000 * D + KINDS.index(kind))
    img = rng.randint(0, 256, size=(3, D, D), dtype=np.uint8)
    img[0, 0, :4] = (0, 255, 0, 255)
    if kind == "mixed":
        img[1] = rng.randint(40, 126, size=(D, D), dtype=np.uint8)
        img[1, 0, :2] = (40, 125)
        img[2] = 77
    return img


def magnitudes(op):
    """torchvision's _augmentation_space(31) of TrivialAugmentWide: (values as Python floats, signed)"""
    import torch

    def linspace(a, b):
        return [float(v) for v in torch.linspace(a, b, 31)]
    if op in (1, 2, 6, 7, 8, 9):
        return linspace(0, 0.99), True
    if op in (3, 4):
        return linspace(0, 32), True
    if op == 5:
        return linspace(0, 135), True
    if op == 10:
        return [float(8 - round(i / 5)) for i in range(31)], False
    if op == 11:
        return linspace(255, 0), False
    return [0.0] * 31, False


def pillow_apply(img, op, bin, neg):
    """img uint8 (3, D, D) -> uint8 (3, D, D): torchvision's _apply_op on the PIL image, fill = None, interpolation NEAREST"""
    pil = Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)), "RGB")
    mags, signed = magnitudes(op)
    m = mags[bin]
    if signed and neg:
        m = -m
    size = pil.size
    if op == 0:
        out = pil
    elif op in (1, 2):
        t = math.tan(math.radians(math.degrees(math.atan(m))))
        out = pil.transform(size, Image.AFFINE, (1.0, t, 0.0, 0.0, 1.0, 0.0) if op == 1 else (1.0, 0.0, 0.0, t, 1.0, 0.0), Image.NEAREST)
    elif op == 3:
        out = pil.transform(size, Image.AFFINE, (1.0, 0.0, float(-int(m)), 0.0, 1.0, 0.0), Image.NEAREST)
    elif op == 4:
        out = pil.transform(size, Image.AFFINE, (1.0, 0.0, 0.0, 0.0, 1.0, float(-int(m))), Image.NEAREST)
    elif op == 5:
        out = pil.rotate(m, Image.NEAREST)
    elif op == 6:
        out = ImageEnhance.Brightness(pil).enhance(1.0 + m)
    elif op == 7:
        out = ImageEnhance.Color(pil).enhance(1.0 + m)
    elif op == 8:
        out = ImageEnhance.Contrast(pil).enhance(1.0 + m)
    elif op == 9:
        out = ImageEnhance.Sharpness(pil).enhance(1.0 + m)
    elif op == 10:
        out = ImageOps.posterize(pil, int(m))
    elif op == 11:
        out = ImageOps.solarize(pil, m)
    elif op == 12:
        out = ImageOps.autocontrast(pil)
    else:
        out = ImageOps.equalize(pil)
    return np.ascontiguousarray(np.asarray(out).transpose(2, 0, 1))


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


if __name__ == "__main__":
    crcs = np.zeros((len(DIMS), len(KINDS), 14, 31, 2), np.uint32)
    for di, D in enumerate(DIMS):
        for ki, kind in enumerate(KINDS):
            img = image(D, kind)
            for op in range(14):
                for b in range(31):
                    for neg in range(2):
                        crcs[di, ki, op, b, neg] = crc(pillow_apply(img, op, b, neg))
    out = {"pillow": np.array(PIL.__version__), "dims": np.array(DIMS), "kinds": np.array(KINDS), "seed": np.array(SEED), "crc": crcs,
           "inputs_crc": np.array([[crc(image(D, k)) for k in KINDS] for D in DIMS], np.uint32), "full": np.array(FULL, dtype=object).astype(str)}
    for j, (D, kind, op, b, neg) in enumerate(FULL):
        out["full%02d" % j] = pillow_apply(image(D, kind), op, b, neg)
    path = os.path.join(HERE, "ta_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d checksums, %d outputs, %d bytes, Pillow %s" % (path, crcs.size, len(FULL), os.path.getsize(path), PIL.__version__))
