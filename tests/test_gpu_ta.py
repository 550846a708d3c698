"""TrivialAugmentWide on its own (include/resnet_mi.h, "TrivialAugmentWide"; ta_stage_kernel and ta_apply_kernel in kernels_input.hip)
through mi_op_trivial_augment, bit for bit against tests/taref.py, which test_ta_model.py pins to Pillow.

One batch of all 14 x 31 x 2 records at D = 30 (16-byte path) and one at D = 33 (odd: every pixel on the scalar path), on three kinds of
images: random bytes (Equalize clips, blends clip on both sides: bytes 0 and 255 are there), a constant channel beside one confined to
40 .. 125 (AutoContrast identity and stretching, Equalize on a single bin), and bytes 0 and 255 only.  D = 7 and 8: smaller than the
translations, and 49 and 64 pixels, so Equalize's step == 0.  n = 1, 3 and 257 (the third launch pair of the by-value records).  Identity
rows and everything behind row n keep their bits, a NaN and -0.0 among them.  A batch that starts 4 bytes into its buffer.  Input that is
no byte (fractions, NaN, +-inf) against the model's quantisation.  A second call over the same workspace.  Behind one sweep of the capped
grid on both paths (mi_debug_ta_geometry).  Every refusal; one run between red zones; one with LDS full of ones."""
import ctypes as C

import numpy as np
import pytest

import taref as R

pytestmark = pytest.mark.gpu

KINDS = ("random", "mixed", "binary")
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _bytes(n, D, kind, seed=0):
    """uint8 (n, 3, D, D); every row its own draw"""
    rng = np.random.RandomState(1000 * D + 10 * n + KINDS.index(kind) + seed)
    b = rng.randint(0, 256, size=(n, 3, D, D), dtype=np.uint8)
    b[:, 0, 0, :2] = (0, 255)
    if kind == "mixed":
        b[:, 1] = rng.randint(40, 126, size=(n, D, D), dtype=np.uint8)
        b[:, 1, 0, :2] = (40, 125)
        b[:, 2] = rng.randint(0, 256, size=(n, 1, 1), dtype=np.uint8)  # a constant channel, another value in every row
    elif kind == "binary":
        b = (b & 1) * np.uint8(255)
        b[:, 0, 0, :2] = (0, 255)
    return b


def all_records(D):
    return [R.row(op, b, neg, D) for op in range(R.N_OPS) for b in range(R.N_BINS) for neg in range(2)]


def _case(D, kind):
    """(images, rows, model's result) of the batch of all records, computed once"""
    if (D, kind) not in _CACHE:
        rows = all_records(D)
        x = R.decode(_bytes(len(rows), D, kind))
        _CACHE[(D, kind)] = (x, rows, R.apply_batch(x, rows))
    return _CACHE[(D, kind)]


def _check(got, want, rows):
    bad = _bits(got) != _bits(want)
    if bad.any():
        r = int(np.flatnonzero(bad.reshape(len(bad), -1).any(axis=1))[0])
        raise AssertionError("%d elements differ from the model, the first in row %d: %s bin %d neg %d" %
                             (int(bad.sum()), r, R.OPS[rows[r]["op"]], rows[r]["bin"], rows[r]["neg"]))


def _names(ops):
    buf = C.create_string_buffer(1 << 14)
    n = ops.L.mi_debug_trace_names(buf, len(buf))
    return [s for s in buf.value.decode().split("\n")[:-1] if s.startswith("ta_")] if n else []


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [30, 33, 7, 8])
def test_every_record(ops, D, kind):
    x, rows, want = _case(D, kind)
    assert len(rows) == 868
    got = ops.trivial_augment(x, rows)
    _check(got, want, rows)
    ident = np.array([r["op"] == R.IDENTITY for r in rows])
    assert _same(got[ident], x[ident])
    assert np.mean(_bits(got)[~ident] != _bits(x)[~ident]) > 0.3  # not vacuous
    if D in (7, 8):  # |translation| >= D: the whole image is byte 0
        far = [i for i, r in enumerate(rows) if r["op"] in (R.TRANSLATE_X, R.TRANSLATE_Y) and abs(r["magnitude"]) >= D + 1]
        assert len(far) > 40 and all(_same(got[i], R.decode(np.zeros((3, D, D), np.uint8))) for i in far)


def test_the_branches_are_taken():
    """the inputs of test_every_record reach what the header names: both clips of the blends, the AutoContrast identity and stretch,
    Equalize on one bin, with step == 0 and with the clip at 255"""
    img = _bytes(868, 30, "random")[0]
    t = np.float32(1.99) * (img.astype(np.float32) - R.luma(img).astype(np.float32)) + R.luma(img).astype(np.float32)
    assert (t <= 0).any() and (t >= 255).any()
    mixed = _bytes(868, 30, "mixed")[0]
    lut_g = R.autocontrast_lut(np.bincount(mixed[1].ravel(), minlength=256))
    assert lut_g[40] == 0 and lut_g[125] == 255 and np.array_equal(R.autocontrast(mixed)[2], mixed[2])
    assert np.array_equal(R.equalize(mixed)[2], mixed[2]) and not np.array_equal(R.equalize(mixed)[0], mixed[0])
    h = np.bincount(img[0].ravel(), minlength=256)
    step = (900 - int(h[np.flatnonzero(h)[-1]])) // 255
    assert step > 0 and (step // 2 + np.cumsum(h)[-2]) // step > 255
    small = _bytes(868, 8, "random")[0]
    assert (64 - np.bincount(small[1].ravel(), minlength=256)[small[1].max()]) // 255 == 0


@pytest.mark.parametrize("D", [8, 33])
@pytest.mark.parametrize("n", [1, 3, 257])
def test_batch_sizes_and_a_drawn_plan(ops, n, D):
    """rows from mi_ta_plan itself; 257 rows: three launch pairs (128 rows a launch)"""
    rows = ops.ta_plan(5, 1, 7, 0, 1, n, D)
    assert [(r["op"], r["bin"], r["neg"], r["arg"], r["A"]) for r in rows] == \
           [(r["op"], r["bin"], r["neg"], r["arg"], r["A"]) for r in R.plan(5, 1, 7, 0, 1, n, D)]
    x = R.decode(_bytes(n, D, "random", seed=3))
    ops.L.mi_debug_trace_clear()
    got = ops.trivial_augment(x, rows)
    _check(got, R.apply_batch(x, rows), rows)
    per = ops.ta_geometry()[2]
    launches = sum(any(r["op"] != R.IDENTITY for r in rows[k:k + per]) for k in range(0, n, per))
    path = "vec" if (D * D) % 4 == 0 else "elem"
    assert _names(ops) == ["ta_stage_kernel<%s>" % path, "ta_apply_kernel<%s>" % path] * launches
    assert launches == {1: 1, 3: 1, 257: 3}[n]  # the seed's rows: no launch of this plan is all identity


def test_a_launch_of_identity_rows_is_skipped(ops):
    D, per = 8, ops.ta_geometry()[2]
    rows = [R.row(R.IDENTITY, 3, 1, D)] * per + [R.row(R.SOLARIZE, 20, 0, D)]
    x = R.decode(_bytes(per + 1, D, "random"))
    ops.L.mi_debug_trace_clear()
    got = ops.trivial_augment(x, rows)
    assert _names(ops) == ["ta_stage_kernel<vec>", "ta_apply_kernel<vec>"]
    _check(got, R.apply_batch(x, rows), rows)
    ops.L.mi_debug_trace_clear()
    assert _same(ops.trivial_augment(x[:5], rows[:5]), x[:5]) and _names(ops) == []


@pytest.mark.parametrize("D", [8, 33])
def test_identity_rows_and_the_rows_behind_n_keep_their_bits(ops, D):
    """NaN words with payloads, -0.0, a subnormal and the largest float in the identity rows and behind row n: no word moves"""
    n = 6
    rows = [R.row(op, 30, 1, D) for op in (R.IDENTITY, R.ROTATE, R.IDENTITY, R.EQUALIZE, R.SHARPNESS, R.IDENTITY)]
    x = np.concatenate([R.decode(_bytes(n, D, "random")), np.zeros((2, 3, D, D), np.float32)])
    for i in (0, 2, 5, 6, 7):
        _bits(x[i]).ravel()[:6] = (0x7FC12345, 0xFF812345, 0x80000000, 0x00000001, 0x7F7FFFFF, 0xFFFFFFFF)
        x[i, 1:] = np.float32(1e30)
    got = ops.trivial_augment(x, rows, n=n)
    _check(got[:n], R.apply_batch(x[:n], rows), rows)
    for i in (0, 2, 5, 6, 7):
        assert _same(got[i], x[i]), i
    assert not _same(got[1], x[1]) and not _same(got[4], x[4]) and (D == 8 or not _same(got[3], x[3]))  # 64 pixels: Equalize's step is 0


@pytest.mark.parametrize("D", [30, 8])
def test_on_an_unaligned_batch(ops, D):
    """the batch starts 4 bytes into a 16-byte aligned buffer: the scalar path although D^2 % 4 == 0"""
    x, rows, want = _case(D, "mixed")
    ops.L.mi_debug_trace_clear()
    got = ops.trivial_augment(x[:100], rows[:100], offset_floats=1)
    assert set(_names(ops)) == {"ta_stage_kernel<elem>", "ta_apply_kernel<elem>"}
    _check(got, want[:100], rows[:100])
    got = ops.trivial_augment(x[400:500], rows[400:500], offset_floats=1)
    _check(got, want[400:500], rows[400:500])


@pytest.mark.parametrize("D", [8, 33])
def test_input_that_is_no_byte_is_rounded(ops, D):
    """fractions (exact halves among them: half to even), values beyond both ends, NaN, +-inf: the model's quantisation"""
    rows = [R.row(op, 12, 0, D) for op in range(1, R.N_OPS)]
    n = len(rows)
    rng = np.random.RandomState(D)
    x = rng.uniform(-150, 200, size=(n, 3, D, D)).astype(np.float32)
    halves = (np.arange(D * D, dtype=np.float32).reshape(D, D) % 256 + np.float32(0.5))
    for d in range(3):
        x[:, d, :, :] = np.where(rng.rand(n, D, D) < 0.3, halves - R.mean_plane(d), x[:, d])
    x[:, 0, 1, :4] = (np.nan, np.inf, -np.inf, -0.0)
    _bits(x[:, 1, 1])[:, :2] = (0xFFC00001, 0x7F800001)
    q = R.quantise(x)
    assert (q == 0).any() and (q == 255).any() and not np.array_equal(R.decode(q), np.where(np.isnan(x), 0, x))
    _check(ops.trivial_augment(x, rows), R.apply_batch(x, rows), rows)


def test_the_statistics_are_rebuilt_on_a_second_call(ops):
    """the same workspace twice, other images the second time: the histograms of the first call are gone"""
    D = 30
    rows = [R.row(op, 30, 0, D) for op in (R.CONTRAST, R.AUTOCONTRAST, R.EQUALIZE, R.CONTRAST, R.EQUALIZE)]
    a, b = R.decode(_bytes(5, D, "random", seed=1)), R.decode(_bytes(5, D, "mixed", seed=2))
    got_a, ws = ops.trivial_augment(a, rows, keep_workspace=True)
    _check(got_a, R.apply_batch(a, rows), rows)
    got_b = ops.trivial_augment(b, rows, workspace=ws)
    _check(got_b, R.apply_batch(b, rows), rows)
    _check(ops.trivial_augment(a, rows, workspace=ws), got_a, rows)


def _sweep_dim(ops, path):
    """the smallest D on `path` whose image is more than one sweep of the capped grid: threads x cap (x 4 on the 16-byte path) pixels"""
    threads, cap, _, quad = ops.ta_geometry()
    D = 1 if path == "elem" else 2
    while D * D <= threads * cap * (1 if path == "elem" else quad):
        D += 2
    return D


@pytest.mark.parametrize("path", ["elem", "vec"])
def test_behind_one_sweep_of_the_grid(ops, path):
    """every operation at its strongest bin, both signs, on an image of more pixels than the capped grid takes in one turn (91 and 182 with
    32 workgroups of 256 threads)"""
    D = _sweep_dim(ops, path)
    assert (D * D) % 4 == (1 if path == "elem" else 0)
    rows = [R.row(op, 30, neg, D) for op in range(R.N_OPS) for neg in range(2)]
    x = R.decode(_bytes(len(rows), D, "random"))
    ops.L.mi_debug_trace_clear()
    got = ops.trivial_augment(x, rows)
    assert _names(ops) == ["ta_stage_kernel<%s>" % path, "ta_apply_kernel<%s>" % path]
    want = R.apply_batch(x, rows)
    _check(got, want, rows)
    threads, cap, _, quad = ops.ta_geometry()
    first = threads * cap * (1 if path == "elem" else quad)
    tail = _bits(got).reshape(len(rows), 3, -1)[2:, :, first:]
    assert np.mean(tail != _bits(x).reshape(len(rows), 3, -1)[2:, :, first:]) > 0.3  # the second turn wrote


def test_bad_arguments(ops):
    from resnet_amd import binding as B
    D, n = 8, 5
    x = R.decode(_bytes(n, D, "random"))
    d = ops.dev(x)
    ws = ops.dev(np.zeros(int(ops.L.mi_ta_workspace_bytes(n, D)) + 16, np.uint8))
    ok = B.ta_rows_struct([R.row(R.SOLARIZE, 10, 0, D)] * n)

    def rows_with(**kw):
        return B.ta_rows_struct([dict(R.row(R.SOLARIZE, 10, 0, D), **kw)] + [R.row(R.SOLARIZE, 10, 0, D)] * (n - 1))
    ops.L.mi_debug_trace_clear()
    cases = [(d.ptr, 0, 192, D, ok, ws.ptr, "n"), (d.ptr, -3, 192, D, ok, ws.ptr, "n"), (d.ptr, 65536, 192, D, ok, ws.ptr, "n"),
             (d.ptr, n, 191, D, ok, ws.ptr, "image_size"), (d.ptr, n, 64, D, ok, ws.ptr, "image_size"), (d.ptr, n, 0, D, ok, ws.ptr, "image_size"),
             (d.ptr, n, 192, 0, ok, ws.ptr, "dim"), (d.ptr, n, 3 * 4097 ** 2, 4097, ok, ws.ptr, "dim"),
             (None, n, 192, D, ok, ws.ptr, "images"), (d.ptr, n, 192, D, None, ws.ptr, "rows"), (d.ptr, n, 192, D, ok, None, "workspace"),
             (d.ptr + 2, n, 192, D, ok, ws.ptr, "aligned"), (d.ptr, n, 192, D, ok, ws.ptr + 4, "aligned"),
             (d.ptr, n, 192, D, rows_with(op=14), ws.ptr, "op"), (d.ptr, n, 192, D, rows_with(op=-1), ws.ptr, "op"),
             (d.ptr, n, 192, D, rows_with(bin=31), ws.ptr, "bin"), (d.ptr, n, 192, D, rows_with(bin=-1), ws.ptr, "bin")]
    for *args, word in cases:
        assert ops.L.mi_op_trivial_augment(*args) == -1, args
        msg = ops.L.mi_last_error().decode()
        ops.L.mi_clear_error()
        assert "trivial_augment" in msg and word in msg, msg
    assert _names(ops) == []  # nothing was launched
    assert _same(d.get(), x)
    assert ops.L.mi_ta_workspace_bytes(0, 8) == 0 and ops.L.mi_ta_workspace_bytes(5, 0) == 0


@pytest.mark.parametrize("D", [8, 7, 33])
def test_stays_inside_its_buffers(ops, D):
    """every operation with the batch and the workspace between two 4096-byte zones of 0xFF; the workspace is exactly
    mi_ta_workspace_bytes long"""
    rows = [R.row(op, 30, neg, D) for op in range(R.N_OPS) for neg in range(2)]
    x = R.decode(_bytes(len(rows), D, "random"))
    plain = ops.trivial_augment(x, rows)
    _check(plain, R.apply_batch(x, rows), rows)
    assert ops.L.mi_debug_redzone(4096, 0xFF) == 0
    try:
        zoned = ops.trivial_augment(x, rows)
        assert ops.L.mi_debug_redzone_check() == 0, ops.L.mi_last_error().decode()
    finally:
        assert ops.L.mi_debug_redzone(0, 0) == 0
    assert _same(zoned, plain)


def test_reads_no_stale_lds(ops):
    """every LDS word 0xFFFFFFFF before each launch: a histogram bin, a table entry or a decode value the workgroup did not write would show"""
    outs = {}
    assert ops.L.mi_debug_lds_fill_mode(1, 0xFFFFFFFF) == 0, ops.L.mi_last_error()
    try:
        for D in (30, 33):
            x, rows, _ = _case(D, "mixed")
            outs[D] = ops.trivial_augment(x[::7], rows[::7])
        assert ops.L.mi_debug_lds_fills() >= 4
    finally:
        assert ops.L.mi_debug_lds_fill_mode(0, 0) == 0
    for D in (30, 33):
        _, rows, want = _case(D, "mixed")
        _check(outs[D], want[::7], rows[::7])
