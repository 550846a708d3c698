"""The mix kernels and the two-label loss head on their own (include/resnet_mi.h, "mixing"; kernels_input.hip, kernels_loss.hip) through
mi_op_mix_batch / mi_op_loss_head_mix, bit for bit against the float32 models of tests/mixref.py.

mixup: n 1, 2, 5, 8 (no pair; one pair; a middle row; more than one pair) x D 7 (image_size 147: every element on the scalar path),
8 (16-byte path), 30 (image_size 2700, a multiple of 4) x lam 0, 1, 0.5, 0.3, and a batch that starts 4 bytes into its buffer.
CutMix at D 30 and 7: empty, whole image, one pixel, x0 = 1 width 5, x0 = 3 width 26, x0 = 4 width 26 (D 30: to the right edge), a box
out of range, an inverted one.
Behind one sweep of the capped grid (mi_debug_mix_geometry: 32768 work items, 512 row segments): mixup at the smallest D whose pair has
more items, CutMix at the smallest D whose boxes have more segments, more than 64 columns and more than 64 16-byte groups per row.
The head on lossref.SHAPES: pred = mi_op_softmax's bits, dlogits = the float32 model's bits on that pred, lam = 1 = mi_op_loss_head's bits,
row_loss inside the bound DESIGN.md ("Loss head") derives, the records, an invalid second label; the batch totals on 130 rows of known
rank (lossref.check_batch_totals); the second weight at a lam where its rounding shows.
"""
import ctypes as C

import numpy as np
import pytest

import lossref
import mixref as R
import synth

pytestmark = pytest.mark.gpu

_IMAGES, _HEAD = {}, {}  # inputs and one-label references: made once, never written


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _images(n, D):
    """U(-124, 152) pixels with the values a blend treats specially: -0.0, +0.0, a subnormal, the largest float"""
    if (n, D) not in _IMAGES:
        x = synth.uniform(77, n * 3 * D * D, -124.0, 152.0, offset=1000 * n + D).reshape(n, 3, D, D).copy()
        x[0, 0, 0, :4] = [-0.0, 0.0, 1e-45, np.finfo(np.float32).max]
        x[-1, 0, 0, :4] = [0.0, -0.0, -1e-45, 1.0]
        _IMAGES[(n, D)] = x
    return _IMAGES[(n, D)]


def _plan(mode, lam=1.0, box=(0, 0, 0, 0)):
    return dict(mode=mode, lam=np.float32(lam), y0=box[0], x0=box[1], y1=box[2], x1=box[3])


@pytest.mark.parametrize("lam", [0.0, 1.0, 0.5, 0.3])
@pytest.mark.parametrize("D", [7, 8, 30])
@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_mixup(ops, n, D, lam):
    x = _images(n, D)
    p = _plan(1, lam)
    got = ops.mix_batch(x, p)
    want = R.mix(x, p)
    assert _same(got, want), "%d elements differ" % int(np.sum(_bits(got) != _bits(want)))
    if n % 2:
        assert _same(got[n // 2], x[n // 2])  # the middle row pairs with itself: not touched
    if lam == 1.0 and n > 1:
        changed = _bits(got) != _bits(x)
        assert np.all(x[changed] == 0) and np.all(_bits(got)[changed] == 0)  # only -0.0 -> +0.0, as the model gives it
    if lam == 0.0 and n > 1:
        assert np.array_equal(got, x[::-1])


def test_mixup_on_an_unaligned_batch(ops):
    """the batch starts 4 bytes into a 16-byte aligned buffer: the per-element path although image_size % 4 == 0"""
    x = _images(5, 8)
    p = _plan(1, 0.3)
    assert _same(ops.mix_batch(x, p, offset_floats=1), R.mix(x, p))
    p = _plan(2, 0.5, (1, 1, 6, 6))
    assert _same(ops.mix_batch(x, p, offset_floats=1), R.mix(x, p))


def _boxes(D):
    return {"empty": (3, 2, 3, 6), "empty_x": (1, 4, 5, 4), "whole": (0, 0, D, D), "pixel": (D - 1, D - 2, D, D - 1), "x1_w5": (2, 1, 6, 6),
            "x3_w26": (0, 3, D - 1, min(29, D)), "x4_w26_edge": (1, min(4, D - 1), D, D), "out_of_range": (-5, -2, D + 7, D + 100), "inverted": (5, 6, 2, 1)}


@pytest.mark.parametrize("box", ["empty", "empty_x", "whole", "pixel", "x1_w5", "x3_w26", "x4_w26_edge", "out_of_range", "inverted"])
@pytest.mark.parametrize("D", [30, 7])
@pytest.mark.parametrize("n", [2, 5])
def test_cutmix(ops, n, D, box):
    x = _images(n, D)
    p = _plan(2, 0.5, _boxes(D)[box])
    got = ops.mix_batch(x, p)
    want = R.mix(x, p)
    assert _same(got, want), "%d elements differ" % int(np.sum(_bits(got) != _bits(want)))
    y0, x0, y1, x1 = R.clamp_box(*_boxes(D)[box], D)
    outside = np.ones((D, D), bool)
    outside[y0:y1, x0:x1] = False
    assert _same(got[:, :, outside], x[:, :, outside])  # elements outside the box keep their bits
    if box in ("empty", "empty_x", "inverted"):
        assert _same(got, x)
    if box in ("whole", "out_of_range"):
        assert _same(got[0], x[n - 1]) and _same(got[n - 1], x[0])


LANES = 64  # a wave takes one row segment of a CutMix box: lane-strided over its elements, or over its 16-byte groups


def _sweeps(ops):
    """what one sweep of the capped grid covers, from the launcher's own constants: work items of a pair (mixup_kernel: 32768), row
    segments of a box (cutmix_kernel: 512).  Everything below them is done before a thread strides on"""
    threads, cap, waves = ops.mix_geometry()
    return threads * cap, cap * waves


def _second_turn_dim(ops, path):
    """the smallest D whose pair has more work items than one sweep: 16-byte groups (3 D^2 / 4 of them, D even) or elements (3 D^2, D odd).
    With 128 workgroups of 256 threads: 210 and 105, 33075 items both"""
    items, _ = _sweeps(ops)
    D = 2 if path != "elem" else 1
    while (3 * D * D // 4 if path != "elem" else 3 * D * D) <= items:
        D += 2
    return D


@pytest.mark.parametrize("path", ["vec", "elem", "vec_unaligned"])
def test_mixup_takes_a_second_grid_stride_turn(ops, path):
    """n = 2 at the smallest D at which the threads of the capped grid stride on (`i += step`), on the 16-byte path, on the element-wise
    path of an odd D, and on the element-wise path of the even D through a batch that starts 4 bytes into its buffer (4 sweeps)"""
    items, _ = _sweeps(ops)
    D = _second_turn_dim(ops, path)
    work = 3 * D * D // 4 if path == "vec" else 3 * D * D
    assert work > items and (3 * D * D) % 4 == (0 if path != "elem" else 3)
    x = _images(2, D)
    p = _plan(1, 0.3)
    got = ops.mix_batch(x, p, offset_floats=1 if path == "vec_unaligned" else 0)
    want = R.mix(x, p)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%d elements differ, the first at flat index %d of %d" % (int(bad.sum()), int(np.flatnonzero(bad.ravel())[0]), bad.size // 2)
    assert np.mean(_bits(got) != _bits(x)) > 0.99  # the comparison is not vacuous: the mix moved (nearly) every element


def _cutmix_dim(ops, path):
    """the smallest D at which the boxes below run every loop of cutmix_kernel more than once.  Both paths: 3 (D - 1) row segments are
    more than one sweep (the segment loop strides on).  elem (D odd): then w >= D - 5 > 2 x 64, three lane turns.  vec (D a multiple of
    16): the narrowest box (w = D - 5, one element in front of the first 16-byte boundary) has more than 64 groups.  With 128 workgroups
    of 4 waves: 173 and 272"""
    _, segments = _sweeps(ops)
    D = 1 if path == "elem" else 16
    while 3 * (D - 1) <= segments or D - 5 <= 2 * LANES or (path == "vec" and (D - 6) // 4 <= LANES):
        D += 2 if path == "elem" else 16
    return D


def _big_boxes(D):
    return {"whole": (0, 0, D, D), "from_1_1": (1, 1, D, D), "x3_inner": (0, 3, D - 1, D - 2)}


@pytest.mark.parametrize("box", ["whole", "from_1_1", "x3_inner"])
@pytest.mark.parametrize("path", ["elem", "vec"])
def test_cutmix_wide_and_tall_boxes(ops, path, box):
    """n = 3 (a middle row).  elem: image_size % 4 != 0, every element on its own, the lanes of a wave take three turns over a row.  vec:
    up to 68 16-byte groups per row (the lanes take a second turn), with 0, 3 and 1 elements in front of them and 0, 0 and 2 behind.
    Every box has more row segments than one sweep of the grid"""
    _, segments = _sweeps(ops)
    D = _cutmix_dim(ops, path)
    assert (3 * D * D) % 4 == (0 if path == "vec" else 3)
    y0, x0, y1, x1 = _big_boxes(D)[box]
    assert 3 * (y1 - y0) > segments and x1 - x0 > 2 * LANES
    x = _images(3, D)
    p = _plan(2, 0.5, (y0, x0, y1, x1))
    got = ops.mix_batch(x, p)
    want = R.mix(x, p)
    inside = np.zeros((D, D), bool)
    inside[y0:y1, x0:x1] = True
    bad = _bits(got[:, :, inside]) != _bits(want[:, :, inside])
    assert not bad.any(), "%d elements inside the box differ from the model" % int(bad.sum())
    assert _same(got[:, :, ~inside], x[:, :, ~inside]), "an element outside the box was written"
    assert _same(got[0][:, inside], x[2][:, inside]) and _same(got[2][:, inside], x[0][:, inside]) and _same(got[1], x[1])
    assert np.mean(_bits(x[0][:, inside]) != _bits(x[2][:, inside])) > 0.99  # not vacuous: the partners differ (nearly) everywhere


def test_mode_0_launches_nothing(ops):
    x = _images(5, 8)
    ops.L.mi_debug_trace_clear()
    assert _same(ops.mix_batch(x, _plan(0, 0.3, (0, 0, 8, 8))), x)
    assert _same(ops.mix_batch(x, _plan(2, 0.3, (2, 2, 2, 8))), x)   # an empty box
    assert _same(ops.mix_batch(x[:1], _plan(1, 0.3)), x[:1])         # no pair
    buf = C.create_string_buffer(1 << 12)
    ops.L.mi_debug_trace_names(buf, len(buf))
    assert "mix" not in buf.value.decode()


@pytest.mark.parametrize("n,D", [(5, 8), (4, 7), (3, 30)])
def test_stays_inside_the_batch(ops, n, D):
    """both modes with every allocation between two 4096-byte zones of 0xFF"""
    x = _images(n, D)
    plans = [_plan(1, 0.3), _plan(2, 0.5, (0, 0, D, D)), _plan(2, 0.5, (-9, 3, D + 9, D + 9)), _plan(2, 0.5, (D - 1, D - 1, D, D))]
    plain = [ops.mix_batch(x, p) for p in plans]
    assert ops.L.mi_debug_redzone(4096, 0xFF) == 0
    try:
        zoned = [ops.mix_batch(x, p) for p in plans]
        assert ops.L.mi_debug_redzone_check() == 0, ops.L.mi_last_error().decode()
    finally:
        assert ops.L.mi_debug_redzone(0, 0) == 0
    assert all(_same(a, b) for a, b in zip(zoned, plain))


def test_reads_no_stale_lds(ops):
    x = _images(5, 8)
    plans = [_plan(1, 0.3), _plan(2, 0.5, (1, 1, 7, 6))]
    plain = [ops.mix_batch(x, p) for p in plans]
    assert ops.L.mi_debug_lds_fill_mode(1, 0xFFFFFFFF) == 0, ops.L.mi_last_error()
    try:
        filled = [ops.mix_batch(x, p) for p in plans]
        assert ops.L.mi_debug_lds_fills() >= 2
    finally:
        assert ops.L.mi_debug_lds_fill_mode(0, 0) == 0
    assert all(_same(a, b) for a, b in zip(filled, plain))


def test_bad_arguments(ops):
    from resnet_amd import binding as B
    x = _images(5, 8)
    d = ops.dev(x)
    plan = B.MiMixPlan(1, 0.5, 0, 0, 0, 0)
    ops.L.mi_debug_trace_clear()
    cases = [(d.ptr, 0, 192, 8, C.byref(plan), "n"), (d.ptr, -3, 192, 8, C.byref(plan), "n"), (d.ptr, 65536, 192, 8, C.byref(plan), "n"),
             (d.ptr, 5, 191, 8, C.byref(plan), "image_size"), (d.ptr, 5, 64, 8, C.byref(plan), "image_size"), (d.ptr, 5, 192, 0, C.byref(plan), "dim"),
             (None, 5, 192, 8, C.byref(plan), "images"), (d.ptr, 5, 192, 8, None, "plan_host"),
             (d.ptr, 5, 192, 8, C.byref(B.MiMixPlan(3, 0.5, 0, 0, 0, 0)), "mode"), (d.ptr, 5, 192, 8, C.byref(B.MiMixPlan(1, 1.5, 0, 0, 0, 0)), "lam"),
             (d.ptr, 5, 192, 8, C.byref(B.MiMixPlan(1, float("nan"), 0, 0, 0, 0)), "lam")]
    for *args, word in cases:
        assert ops.L.mi_op_mix_batch(*args) == -1, args
        msg = ops.L.mi_last_error().decode()
        ops.L.mi_clear_error()
        assert "mix_batch" in msg and word in msg, msg
    buf = C.create_string_buffer(1 << 12)
    ops.L.mi_debug_trace_names(buf, len(buf))
    assert "mix" not in buf.value.decode()  # nothing was launched
    assert _same(d.get(), x)


# ---------------------------------------------------------------- the two-label head
def _head_case(ops, shape):
    if shape not in _HEAD:
        x, a = lossref.make_inputs(*shape)
        _HEAD[shape] = (x, a, R.labels_b(a), ops.softmax(x))
    return _HEAD[shape]


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("lam", R.LAMS)
@pytest.mark.parametrize("shape", lossref.SHAPES)
def test_loss_head_mix(ops, shape, lam, eps):
    from resnet_amd import binding as B
    N, L = shape
    x, a, rev, sm = _head_case(ops, shape)
    k = min(5, L)
    lam32 = np.float32(lam)
    one = ops.loss_head(x, a, eps, k) if lam == 1.0 else None
    for b in (rev, a):  # the partner's label (a != b in most rows), and a == b
        total = ops.dev(np.zeros(C.sizeof(B.MiLossMetrics), np.uint8))
        pred, dl, rl, rr, last, tot = ops.loss_head_mix(x, a, b, lam32, eps, k, total=total)
        assert _same(pred, sm), "pred differs from mi_op_softmax"
        want_dl = pred - R.targets_f32(L, a, b, lam32, eps)
        assert _same(dl, want_dl), "dlogits: %d elements differ from the float32 model" % int(np.sum(_bits(dl) != _bits(want_dl)))
        assert np.array_equal(rr, lossref.rank_of(pred, a))  # the rank is label a's
        if one is not None:  # lam = 1.f: the one-label head's bits, whatever labels_b holds
            assert _same(pred, one[0]) and _same(dl, one[1]) and np.array_equal(rr, one[3])
        ref = R.loss_head_mix(x, a, b, lam32, eps)[2]
        err = np.abs(rl.astype(np.float64) - ref)
        print("row_loss %s lam %g eps %g: worst |error| / bound = %.4f" % (shape, lam, eps, float(np.max(err / lossref.loss_bound(ref)))))
        assert np.all(np.isfinite(rl))
        assert np.all(err <= lossref.loss_bound(ref)), (err, lossref.loss_bound(ref))
        want = float(np.sum(rl.astype(np.float64)))
        assert abs(last["loss_sum"] - want) <= 1e-12 * abs(want)
        assert (last["rows"], last["wrong_top1"], last["wrong_topk"], last["batches"]) == (N, int(np.sum(rr >= 1)), int(np.sum(rr >= k)), 1)
        assert tot == last
        again = ops.loss_head_mix(x, a, b, lam32, eps, k, total=total)
        assert _same(again[0], pred) and _same(again[1], dl) and _same(again[2], rl) and again[4] == last
        assert again[5]["loss_sum"] == 2 * last["loss_sum"] and again[5]["batches"] == 2


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("topk", [1, 5, 10])
def test_batch_totals_past_64_rows_and_at_the_topk_threshold(ops, topk, eps):
    """loss_reduce_kernel behind the two-label head (lossref.check_batch_totals says what is built and asserted); the rank is label a's"""
    from resnet_amd import binding as B
    lam = np.float32(0.3)
    new_total = lambda: ops.dev(np.zeros(C.sizeof(B.MiLossMetrics), np.uint8))
    pred, dl, rl = lossref.check_batch_totals(lambda x, a, total: ops.loss_head_mix(x, a, R.labels_b(a), lam, eps, topk, total=total), new_total, topk)
    x, a, _ = lossref.ranked_inputs()
    assert _same(pred, ops.softmax(x)) and _same(dl, pred - R.targets_f32(x.shape[1], a, R.labels_b(a), lam, eps))
    ref = R.loss_head_mix(x, a, R.labels_b(a), lam, eps)[2]
    assert np.all(np.abs(rl.astype(np.float64) - ref) <= lossref.loss_bound(ref))


def test_second_weight_is_one_rounded_product(ops):
    """wb = (1.f - eps) (x) (1.f - lam), rounded once.  At the weights of test_loss_head_mix every other way of forming it gives the same
    float32 (mixref.WB_LAM says so); at lam = 0.7, eps = 0.1 the difference (1.f - eps) - wa is the neighbouring float, and every row's
    t_b -- and t_a where a == b -- shows it"""
    shape = (3, 10)
    x, a, rev, sm = _head_case(ops, shape)
    lam, eps = np.float32(R.WB_LAM), R.WB_EPS
    assert R.wb_as_difference(lam, eps) != (np.float32(1) - np.float32(eps)) * (np.float32(1) - lam)
    for b in (rev, a):
        pred, dl, rl, rr, _, _ = ops.loss_head_mix(x, a, b, lam, eps, 5)
        want = pred - R.targets_f32(shape[1], a, b, lam, eps)
        assert _same(pred, sm)
        assert _same(dl, want), "dlogits: %d elements differ from the float32 model" % int(np.sum(_bits(dl) != _bits(want)))
        ref = R.loss_head_mix(x, a, b, lam, eps)[2]
        assert np.all(np.abs(rl.astype(np.float64) - ref) <= lossref.loss_bound(ref))


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("shape", [(3, 10), (4, 65), (7, 1537)])
def test_second_label_outside_the_row(ops, shape, eps):
    N, L = shape
    x, a, rev, sm = _head_case(ops, shape)
    bad = rev.copy()
    bad[0], bad[-1] = -1, L
    lam = np.float32(0.3)
    good = ops.loss_head_mix(x, a, rev, lam, eps, min(5, L))
    pred, dl, rl, rr, last, _ = ops.loss_head_mix(x, a, bad, lam, eps, min(5, L))
    assert _same(pred, sm) and np.array_equal(rr, good[3])
    assert _same(dl, pred - R.targets_f32(L, a, bad, lam, eps))  # rows 0 and N - 1: no t_b term
    assert np.isnan(rl[0]) and np.isnan(rl[-1]) and _same(rl[1:-1], good[2][1:-1]) and np.isnan(last["loss_sum"])
    # wb == 0: labels_b is not looked at
    one = ops.loss_head(x, a, eps, min(5, L))
    got = ops.loss_head_mix(x, a, bad, np.float32(1.0), eps, min(5, L))
    assert _same(got[0], one[0]) and _same(got[1], one[1]) and np.array_equal(got[3], one[3]) and np.all(np.isfinite(got[2]))
    # a outside the row: as the one-label head
    bad_a = a.copy()
    bad_a[0] = L
    got = ops.loss_head_mix(x, bad_a, rev, lam, eps, min(5, L))
    assert got[3][0] == L and np.isnan(got[2][0]) and _same(got[1], pred - R.targets_f32(L, bad_a, rev, lam, eps))


@pytest.mark.parametrize("shape", [(3, 10), (4, 65)])
def test_head_stays_inside_its_tensors(ops, shape):
    N, L = shape
    x, a, rev, _ = _head_case(ops, shape)
    bad = rev.copy()
    bad[0], bad[-1] = -1, L
    plain = [ops.loss_head_mix(x, a, b, np.float32(0.3), 0.1, min(5, L)) for b in (rev, bad)]
    assert ops.L.mi_debug_redzone(4096, 0xFF) == 0
    try:
        zoned = [ops.loss_head_mix(x, a, b, np.float32(0.3), 0.1, min(5, L)) for b in (rev, bad)]
        assert ops.L.mi_debug_redzone_check() == 0, ops.L.mi_last_error().decode()
    finally:
        assert ops.L.mi_debug_redzone(0, 0) == 0
    for z, p in zip(zoned, plain):
        assert _same(z[0], p[0]) and _same(z[1], p[1]) and _same(z[2], p[2]) and np.array_equal(z[3], p[3])


@pytest.mark.parametrize("lam,word", [(1.5, "lam"), (-0.1, "lam"), (float("nan"), "lam")])
def test_head_bad_arguments(ops, lam, word):
    x, a, rev, _ = _head_case(ops, (4, 65))
    dx, da, db, dp = ops.dev(x), ops.dev(a), ops.dev(rev), ops.dev(shape=x.shape)
    before = dp.get()
    assert ops.L.mi_op_loss_head_mix(dx.ptr, da.ptr, db.ptr, lam, dp.ptr, None, None, None, 4, 65, 0.1, 5, None, None) == -1
    msg = ops.L.mi_last_error().decode()
    ops.L.mi_clear_error()
    assert "mi_op_loss_head_mix" in msg and word in msg, msg
    assert ops.L.mi_op_loss_head_mix(dx.ptr, da.ptr, None, 0.5, dp.ptr, None, None, None, 4, 65, 0.1, 5, None, None) == -1
    assert "labels_b" in ops.L.mi_last_error().decode()
    ops.L.mi_clear_error()
    assert _same(dp.get(), before)
