"""Writes tests/golden/aa_golden.npz from Pillow: seeded uint8 images, a box each, and img.crop(box).resize((V, V), BILINEAR) as Pillow
computes it.  The fixture pins tests/aaref.py where Pillow is not installed.  python tests/golden/make_aa_golden.py"""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = 40


def pillow_resize(img, box, V):
    """img uint8 (H, W, 3), box (row0, col0, h, w) -> uint8 (V, V, 3)"""
    r0, c0, h, w = (int(v) for v in box)
    return np.asarray(Image.fromarray(img).crop((c0, r0, c0 + w, r0 + h)).resize((V, V), Image.BILINEAR))


def cases(count, rng, max_in, max_out):
    """(img, box, V): image sides 8 .. max_in, boxes down to one pixel, outputs 1 .. max_out -- up- and downscales, up to max_in taps"""
    for k in range(count):
        H, W = rng.randint(8, max_in + 1, size=2)
        img = rng.randint(0, 256, size=(H, W, 3), dtype=np.uint8)
        h = 1 if k % 7 == 0 else rng.randint(1, H + 1)
        w = 1 if k % 11 == 0 else rng.randint(1, W + 1)
        V = (1, 2, 3)[k % 3] if k % 13 == 0 else rng.randint(1, max_out + 1)
        yield img, (rng.randint(0, H - h + 1), rng.randint(0, W - w + 1), h, w), V


if __name__ == "__main__":
    out = {"pillow": np.array(PIL.__version__), "n": np.array(CASES)}
    for k, (img, box, V) in enumerate(cases(CASES, np.random.RandomState(20261020), 32, 40)):
        out["img%02d" % k], out["box%02d" % k], out["res%02d" % k] = img, np.array(box, np.int32), pillow_resize(img, box, V)
    path = os.path.join(HERE, "aa_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d cases, %d bytes, Pillow %s" % (path, CASES, os.path.getsize(path), PIL.__version__))
