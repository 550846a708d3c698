"""The erase kernel on its own (include/resnet_mi.h, "random erasing"; kernels_input.hip) through mi_op_erase_batch, bit for bit against
tests/eraseref.py, in both fill modes.

Images as test_gpu_mix._images makes them (-0.0, a subnormal, the largest float), with a NaN of a chosen payload in every row that has an
element outside its box.  n 1, 3, 8 x D 7 (image_size 147: every store on the scalar path), 8 and 30, every row with a box of its own:
none, empty by h, empty by w, one pixel, the whole image, x0 = 1 width 5, x0 = 3 width 26, x0 = 4 width 26 to the right edge, boxes out of
range (sizes past 16 bits, an origin behind the image), a negative origin; all of them in one launch at n = 11.  A batch that starts
4 bytes into its buffer.  n = 257, the second launch of the by-value plan.  Behind one sweep of the capped grid (mi_debug_erase_geometry).
NOISE: a box and a sub-box agree on the common pixels; first_row carries on.  The refusals; one run between red zones.
"""
import ctypes as C

import numpy as np
import pytest

import eraseref as R

pytestmark = pytest.mark.gpu

MODES = ["const", "noise"]
# CONST stores words: -0.0 and a subnormal must arrive as they are.  NOISE: a std of 0 under a value of -0.0 gives -0.0 + (+-0.0)
FILL = {"const": dict(value=(-0.0, 3.5, 1e-45), std=(1.0, 1.0, 1.0)),
        "noise": dict(value=(10.3, -0.0, 5.0), std=(58.395, 0.0, 1e-3), noise_seed=0x9E3779B97F4A7C15)}
KINDS = ["none", "empty_h", "empty_w", "pixel", "whole", "x1_w5", "x3_w26", "x4_w26_edge", "out_of_range", "behind", "negative_origin"]
NAN_WORDS = (0x7FC12345, 0xFF812345)  # a quiet and a signalling NaN with payloads


def _box(kind, D):
    return {"none": (0, 0, 0, 0), "empty_h": (3, 2, 0, 4), "empty_w": (1, 4, 3, 0), "pixel": (D - 1, D - 2, 1, 1), "whole": (0, 0, D, D),
            "x1_w5": (2, 1, 4, 5), "x3_w26": (0, 3, D - 1, min(26, D - 3)), "x4_w26_edge": (1, min(4, D - 1), D - 1, 26),
            "out_of_range": (2, 3, 70000, 2 ** 31 - 1), "behind": (D + 5, 1, 3, 3), "negative_origin": (-3, -2, 5, 4)}[kind]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _outside(boxes, n, D):
    m = np.ones((n, 3, D, D), bool)
    for i in range(n):
        y0, x0, h, w = R.clamp_box(*boxes[i], D)
        m[i, :, y0:y0 + h, x0:x0 + w] = False
    return m


def _images(n, D, boxes):
    """test_gpu_mix's images (shared, never written: a copy) with two NaN words in each row's first elements outside its box"""
    from test_gpu_mix import _images as mix_images
    x = mix_images(n, D).copy()
    out = _outside(boxes, n, D)
    for i in range(n):
        at = np.flatnonzero(out[i].ravel())[5:7]  # behind the special values of rows 0 and n - 1
        _bits(x[i]).ravel()[at] = NAN_WORDS[:len(at)]
    return x


def _check(ops, x, boxes, mode, **kw):
    n, D = x.shape[0], x.shape[2]
    fill = dict(FILL[mode], **{k: v for k, v in kw.items() if k in ("noise_seed", "first_row")})
    got = ops.erase_batch(x, boxes, mode, offset_floats=kw.get("offset_floats", 0), **fill)
    want = R.erase(x, boxes, mode, **fill)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%d elements differ from the model, the first at flat index %d" % (int(bad.sum()), int(np.flatnonzero(bad.ravel())[0]))
    out = _outside(boxes, n, D)
    assert np.array_equal(_bits(got)[out], _bits(x)[out])  # every word outside the boxes keeps its bits
    return got


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("first", [0, 4, 8])
@pytest.mark.parametrize("D", [7, 8, 30])
@pytest.mark.parametrize("n", [1, 3, 8])
def test_erase(ops, n, D, first, mode):
    kinds = [KINDS[(first + i) % len(KINDS)] for i in range(n)]
    boxes = [_box(k, D) for k in kinds]
    x = _images(n, D, boxes)
    got = _check(ops, x, boxes, mode)
    for i, k in enumerate(kinds):
        if k in ("none", "empty_h", "empty_w", "behind"):
            assert _same(got[i], x[i]), k
        if k == "whole" and mode == "const":
            assert all(np.all(_bits(got[i, c]) == _bits(np.float32(FILL["const"]["value"][c]))) for c in range(3))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [7, 8, 30])
def test_every_box_kind_in_one_launch(ops, D, mode):
    boxes = [_box(k, D) for k in KINDS]
    x = _images(len(KINDS), D, boxes)
    got = _check(ops, x, boxes, mode)
    assert np.isnan(got).sum() >= 2 * (len(KINDS) - 2) and not _same(got, x)  # the NaN words outside the boxes are still there


@pytest.mark.parametrize("mode", MODES)
def test_on_an_unaligned_batch(ops, mode):
    """the batch starts 4 bytes into a 16-byte aligned buffer: the per-element path although image_size % 4 == 0"""
    D = 8
    boxes = [_box(k, D) for k in ("x1_w5", "whole", "negative_origin", "none", "pixel")]
    x = _images(5, D, boxes)
    ops.L.mi_debug_trace_clear()
    _check(ops, x, boxes, mode, offset_floats=1)
    assert _names(ops) == ["erase_kernel<%s,elem>" % mode]


def _names(ops):
    buf = C.create_string_buffer(1 << 12)
    n = ops.L.mi_debug_trace_names(buf, len(buf))
    return [s for s in buf.value.decode().split("\n")[:-1] if "erase" in s] if n else []


@pytest.mark.parametrize("mode", MODES)
def test_launch_names_and_the_launch_without_boxes(ops, mode):
    ops.L.mi_debug_trace_clear()
    for D, path in ((8, "vec"), (7, "elem")):
        boxes = [_box("x1_w5", D), _box("none", D), _box("pixel", D)]
        _check(ops, _images(3, D, boxes), boxes, mode)
    assert _names(ops) == ["erase_kernel<%s,vec>" % mode, "erase_kernel<%s,elem>" % mode]
    ops.L.mi_debug_trace_clear()
    boxes = [_box(k, 8) for k in ("none", "empty_h", "empty_w", "behind")]
    x = _images(4, 8, boxes)
    assert _same(_check(ops, x, boxes, mode), x)
    assert _names(ops) == []  # no row has a box: nothing is launched


@pytest.mark.parametrize("mode", MODES)
def test_the_second_launch_of_the_by_value_plan(ops, mode):
    """n = 257 at D = 8: the boxes travel 256 rows a launch.  Rows 0, 255 and 256 carry boxes (the last row of the first launch, the only
    row of the second); in NOISE mode row 256's key index is first_row + 256"""
    rows = ops.erase_geometry()[3]
    n, D = rows + 1, 8
    boxes = np.zeros((n, 4), np.int32)
    boxes[0], boxes[rows - 1], boxes[rows] = (1, 1, 3, 5), (0, 0, D, D), (2, 1, 5, 6)
    x = _images(n, D, boxes)
    ops.L.mi_debug_trace_clear()
    got = _check(ops, x, boxes, mode, first_row=1000)
    assert len(_names(ops)) == 2
    assert not _same(got[rows], x[rows]) and not _same(got[rows - 1], x[rows - 1])
    # boxes in the second launch only: the first is skipped
    boxes[:rows] = 0
    ops.L.mi_debug_trace_clear()
    _check(ops, x, boxes, mode, first_row=1000)
    assert len(_names(ops)) == 1


LANES = 64  # a wave takes one row segment of a box: lane-strided over its elements, or over its 16-byte groups


def _sweep_dim(ops, path):
    """the smallest D at which the boxes below run every loop of erase_kernel more than once.  Both paths: 3 (D - 1) row segments are more
    than one sweep of the capped grid.  elem (D odd): w >= D - 5 > 2 x 64, three lane turns.  vec (D a multiple of 16): the narrowest box
    (w = D - 5, one element in front of the first 16-byte boundary) has more than 64 groups.  With 128 workgroups of 4 waves: 173 and 272"""
    _, cap, waves, _ = ops.erase_geometry()
    D = 1 if path == "elem" else 16
    while 3 * (D - 1) <= cap * waves or D - 5 <= 2 * LANES or (path == "vec" and (D - 6) // 4 <= LANES):
        D += 2 if path == "elem" else 16
    return D


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["elem", "vec"])
def test_wide_and_tall_boxes(ops, path, mode):
    """three rows, three boxes: the whole image, from (1, 1) to the far corner, columns 3 .. D - 3 of all rows but the last: up to 68 16-byte
    groups per row segment with 0, 3 and 1 elements in front of them, and more row segments than one sweep of the grid in every row"""
    _, cap, waves, _ = ops.erase_geometry()
    D = _sweep_dim(ops, path)
    assert (3 * D * D) % 4 == (0 if path == "vec" else 3)
    boxes = [(0, 0, D, D), (1, 1, D - 1, D - 1), (0, 3, D - 1, D - 5)]
    assert all(3 * b[2] > cap * waves and b[3] > 2 * LANES for b in boxes)
    x = _images(3, D, boxes)
    ops.L.mi_debug_trace_clear()
    got = _check(ops, x, boxes, mode)
    assert _names(ops) == ["erase_kernel<%s,%s>" % (mode, path)]
    inside = ~_outside(boxes, 3, D)
    assert np.mean(_bits(got)[inside] != _bits(x)[inside]) > 0.99  # not vacuous: the fill moved (nearly) every element of the boxes


def test_noise_is_a_function_of_the_position(ops):
    """a box and a sub-box of it give equal bits on the common pixels; first_row = 5 on 3 rows equals rows 5 .. 7 of an 8-row call"""
    D = 30
    from test_gpu_mix import _images as mix_images
    x = mix_images(8, D)
    big = ops.erase_batch(x, [(2, 1, 20, 27)] * 8, "noise", **FILL["noise"])
    small = ops.erase_batch(x, [(5, 4, 9, 13)] * 8, "noise", **FILL["noise"])
    assert _same(big[:, :, 5:14, 4:17], small[:, :, 5:14, 4:17])
    assert not _same(big[0, :, 5:14, 4:17], big[1, :, 5:14, 4:17])  # a row has its own key
    part = ops.erase_batch(x[5:8], [(2, 1, 20, 27)] * 3, "noise", first_row=5, **FILL["noise"])
    assert _same(part, big[5:8])
    assert not _same(ops.erase_batch(x[5:8], [(2, 1, 20, 27)] * 3, "noise", first_row=0, **FILL["noise"]), big[5:8])
    other = dict(FILL["noise"], noise_seed=1)
    assert not _same(ops.erase_batch(x, [(2, 1, 20, 27)] * 8, "noise", **other), big)


def test_bad_arguments(ops):
    from resnet_amd import binding as B
    from test_gpu_mix import _images as mix_images
    x = mix_images(5, 8)
    d = ops.dev(x)
    boxes = np.tile(np.array([0, 0, 8, 8], np.int32), (5, 1))
    bp = boxes.ctypes.data
    ok = B.erase_fill_struct("noise")
    nan, inf = float("nan"), float("inf")
    ops.L.mi_debug_trace_clear()
    cases = [(d.ptr, 0, 192, 8, bp, C.byref(ok), 0, "n"), (d.ptr, -3, 192, 8, bp, C.byref(ok), 0, "n"), (d.ptr, 65536, 192, 8, bp, C.byref(ok), 0, "n"),
             (d.ptr, 5, 191, 8, bp, C.byref(ok), 0, "image_size"), (d.ptr, 5, 64, 8, bp, C.byref(ok), 0, "image_size"),
             (d.ptr, 5, 192, 0, bp, C.byref(ok), 0, "dim"), (d.ptr, 5, 3 * 16385 ** 2, 16385, bp, C.byref(ok), 0, "dim"),
             (None, 5, 192, 8, bp, C.byref(ok), 0, "images"), (d.ptr, 5, 192, 8, None, C.byref(ok), 0, "boxes"), (d.ptr, 5, 192, 8, bp, None, 0, "fill_host"),
             (d.ptr + 2, 5, 192, 8, bp, C.byref(ok), 0, "aligned"),
             (d.ptr, 5, 192, 8, bp, C.byref(B.erase_fill_struct(2)), 0, "mode"), (d.ptr, 5, 192, 8, bp, C.byref(B.erase_fill_struct(-1)), 0, "mode"),
             (d.ptr, 5, 192, 8, bp, C.byref(B.erase_fill_struct("const", value=(0, nan, 0))), 0, "finite"),
             (d.ptr, 5, 192, 8, bp, C.byref(B.erase_fill_struct("const", value=(inf, 0, 0))), 0, "finite"),
             (d.ptr, 5, 192, 8, bp, C.byref(B.erase_fill_struct("noise", std=(1, 1, inf))), 0, "finite"),
             (d.ptr, 5, 192, 8, bp, C.byref(B.erase_fill_struct("noise", std=(1, -0.5, 1))), 0, "negative")]
    for *args, word in cases:
        assert ops.L.mi_op_erase_batch(*args) == -1, args
        msg = ops.L.mi_last_error().decode()
        ops.L.mi_clear_error()
        assert "erase_batch" in msg and word in msg, msg
    assert _names(ops) == []  # nothing was launched
    assert _same(d.get(), x)


@pytest.mark.parametrize("n,D", [(5, 8), (4, 7), (3, 30)])
def test_stays_inside_the_batch(ops, n, D):
    """both modes with every allocation between two 4096-byte zones of 0xFF, boxes out of range in every row"""
    boxes = [_box(k, D) for k in ("out_of_range", "negative_origin", "behind", "whole", "x4_w26_edge")][:n]
    x = _images(n, D, boxes)
    plain = [_check(ops, x, boxes, m) for m in MODES]
    assert ops.L.mi_debug_redzone(4096, 0xFF) == 0
    try:
        zoned = [ops.erase_batch(x, boxes, m, **FILL[m]) for m in MODES]
        assert ops.L.mi_debug_redzone_check() == 0, ops.L.mi_last_error().decode()
    finally:
        assert ops.L.mi_debug_redzone(0, 0) == 0
    assert all(_same(a, b) for a, b in zip(zoned, plain))
