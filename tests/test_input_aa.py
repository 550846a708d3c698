"""The antialiased resize off the device (include/resnet_mi.h, "antialiased resize"): the numpy model (tests/aaref.py) against Pillow
itself and against the fixture Pillow wrote (tests/golden/aa_golden.npz), and the library's tap table mi_aa_coeffs -- compiled from the
text the kernel compiles -- against the model's.  CPU only; everything is compared bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

import aaref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "aa_golden.npz")


def model_resize(img, box, V):
    r0, c0, h, w = (int(v) for v in box)
    return aaref.resize(img[r0:r0 + h, c0:c0 + w, :], V)


def test_model_equals_pillow_on_a_seeded_sweep():
    pytest.importorskip("PIL")
    spec = importlib.util.spec_from_file_location("make_aa_golden", os.path.join(HERE, "golden", "make_aa_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    most_taps, shapes = 0, set()
    for k, (img, box, V) in enumerate(mk.cases(300, np.random.RandomState(7), 96, 64)):
        want, got = mk.pillow_resize(img, box, V), model_resize(img, box, V)
        assert got.shape == want.shape and np.array_equal(got, want), (k, img.shape, box, V, np.argwhere(got != want)[:1])
        most_taps = max(most_taps, max(len(aaref.taps(box[2], V, o)[1]) for o in range(V)))
        shapes.add((box[2] > V, box[3] > V))
    assert most_taps >= 40 and len(shapes) == 4  # strong downscales, and up / down on either axis in every combination
    # the validation resize: 256 -> 232, the centre 224^2 of it
    img = np.random.RandomState(8).randint(0, 256, size=(256, 256, 3), dtype=np.uint8)
    want, got = mk.pillow_resize(img, (0, 0, 256, 256), 232), model_resize(img, (0, 0, 256, 256), 232)
    assert np.array_equal(got, want) and np.array_equal(got[4:228, 4:228], want[4:228, 4:228])


def test_model_equals_the_fixture_pillow_wrote():
    g = np.load(GOLD)
    n = int(g["n"])
    assert n >= 36 and os.path.getsize(GOLD) < 200 * 1024
    kinds = set()
    for k in range(n):
        img, box, want = g["img%02d" % k], g["box%02d" % k], g["res%02d" % k]
        got = model_resize(img, box, want.shape[0])
        assert got.shape == want.shape and np.array_equal(got, want), (k, img.shape, box, want.shape)
        kinds.add((box[2] > want.shape[0], box[3] > want.shape[0]))
    assert len(kinds) == 4


def test_skipped_pass_is_the_table_that_hands_bytes_through():
    """in == V: Pillow skips the pass; the table K = (2^22, 0) the kernel runs instead gives the same bytes"""
    for n in (1, 2, 7, 224):
        m = aaref.table(n, n)
        assert np.array_equal(m, np.eye(n, dtype=np.int64) << 22)


def c_taps(lib, length, V, o, cap):
    K = np.full(cap + 2, -77, np.int32)
    xmin = np.array([-5], np.int32)
    n = lib.mi_aa_coeffs(length, V, o, xmin.ctypes.data, K.ctypes.data, cap)
    return n, int(xmin[0]), K


GRID = [(i, v) for i in (1, 2, 7, 8, 33, 96, 256) for v in (1, 4, 7, 24, 176, 224, 232)]
LONG = [(16384, 1), (16384, 7), (16384, 224), (16384, 16383), (1, 16384), (224, 16384), (16383, 16384)]


@pytest.mark.parametrize("length,V", GRID + LONG)
def test_mi_aa_coeffs_is_the_models_table(length, V):
    from resnet_amd import binding as B
    lib = B.load()
    cap = aaref.ksize(length, V)
    outs = range(V) if V <= 256 else sorted(set(np.random.RandomState(V).randint(0, V, 200).tolist() + [0, 1, V // 2, V - 2, V - 1]))
    for o in outs:
        xmin, K = aaref.taps(length, V, o)
        n, cx, cK = c_taps(lib, length, V, o, cap)
        assert 1 <= n <= cap and (n, cx) == (len(K), xmin), (o, n, cx, len(K), xmin)
        assert np.array_equal(cK[:n], K), (o, np.argwhere(cK[:n] != K)[:1])
        assert np.all(cK[n:] == -77)  # nothing behind the taps is written
        assert abs(int(K.sum()) - (1 << 22)) <= n and 255 * int(K.sum()) + (1 << 21) < 2 ** 31


def test_mi_aa_coeffs_honours_cap_and_refuses_nonsense():
    from resnet_amd import binding as B
    lib = B.load()
    xmin, K = aaref.taps(96, 7, 3)
    n, cx, cK = c_taps(lib, 96, 7, 3, 5)
    assert n == len(K) > 5 and cx == xmin and np.array_equal(cK[:5], K[:5]) and np.all(cK[5:] == -77)
    for bad in ((0, 4, 0), (4, 0, 0), (4, 4, 4), (4, 4, -1)):
        assert c_taps(lib, *bad, 8)[0] == -1
        assert "mi_aa_coeffs" in lib.mi_last_error().decode()
        lib.mi_clear_error()
