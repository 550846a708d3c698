"""TrivialAugmentWide without a GPU (include/resnet_mi.h, "TrivialAugmentWide"): the numpy model tests/taref.py against Pillow's own calls
(byte equality; skipped only where Pillow is missing) and, always, against the fixture Pillow wrote (tests/golden/ta_golden.npz); the
library's mi_ta_row and mi_ta_plan -- host code, loads without a GPU -- against the model field by field; the committed magnitude tables
against torch.linspace; quantise o decode on all 3 x 256 table values; the plan's uniformity and its independence of the erase and mix
plans."""
import ctypes as C
import importlib.util
import math
import os
import zlib

import numpy as np
import pytest

import eraseref
import taref as R
from mixref import M64, splitmix64_at

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "ta_golden.npz")
KINDS = ("random", "mixed")
SEED = 20261021


def image(D, kind):
    """make_ta_golden.image restated (the fixture's inputs_crc holds the two together)"""
    rng = np.random.RandomState(SEED + 1000 * D + KINDS.index(kind))
    img = rng.randint(0, 256, size=(3, D, D), dtype=np.uint8)
    img[0, 0, :4] = (0, 255, 0, 255)
    if kind == "mixed":
        img[1] = rng.randint(40, 126, size=(D, D), dtype=np.uint8)
        img[1, 0, :2] = (40, 125)
        img[2] = 77
    return img


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    from resnet_amd import binding
    return binding.load()


@pytest.fixture(scope="module")
def pillow():
    pytest.importorskip("PIL")
    spec = importlib.util.spec_from_file_location("make_ta_golden", os.path.join(HERE, "golden", "make_ta_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---- the model against Pillow ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("D", [30, 33])
def test_model_equals_pillow_on_every_record(pillow, D, kind):
    """every op x all 31 bins x both signs"""
    img = image(D, kind)
    assert np.array_equal(img, pillow.image(D, kind))
    changed = 0
    for op in range(R.N_OPS):
        for b in range(R.N_BINS):
            for neg in range(2):
                want, got = pillow.pillow_apply(img, op, b, neg), R.apply(img, R.row(op, b, neg, D))
                assert np.array_equal(want, got), (R.OPS[op], b, neg, int((want != got).sum()))
                changed += not np.array_equal(got, img)
    assert changed > 600  # not vacuous: nearly every record outside Identity moves the image


@pytest.mark.parametrize("D", [7, 8, 224])
def test_model_equals_pillow_on_a_sample_of_sizes(pillow, D):
    """7 and 8: smaller than the translations, 49 and 64 pixels (Equalize's step == 0); 224: the recipe's size"""
    for kind in KINDS:
        img = image(D, kind)
        for op in range(R.N_OPS):
            for b in (0, 7, 16, 30) if D == 224 else range(0, R.N_BINS, 3):
                for neg in range(2):
                    want, got = pillow.pillow_apply(img, op, b, neg), R.apply(img, R.row(op, b, neg, D))
                    assert np.array_equal(want, got), (D, kind, R.OPS[op], b, neg)


@pytest.mark.parametrize("D", [17, 30, 33])
def test_equalize_clips_as_pillow_does(pillow, D):
    """random images of 17^2, 30^2 and 33^2 pixels push n / step past 255"""
    img = np.random.RandomState(D).randint(0, 256, size=(3, D, D), dtype=np.uint8)
    h = np.bincount(img[0].ravel(), minlength=256)
    step = (int(h.sum()) - int(h[np.flatnonzero(h)[-1]])) // 255
    assert step > 0 and int((step // 2 + np.cumsum(h)[-2]) // step) > 255  # the clip is needed
    assert np.array_equal(pillow.pillow_apply(img, R.EQUALIZE, 0, 0), R.equalize(img))


# ---- the model against the fixture ----
def test_model_equals_the_fixture():
    g = np.load(GOLD)
    assert tuple(g["dims"]) == (30, 33) and tuple(g["kinds"]) == KINDS and int(g["seed"]) == SEED
    assert g["crc"].shape == (2, 2, R.N_OPS, R.N_BINS, 2)
    for di, D in enumerate((30, 33)):
        for ki, kind in enumerate(KINDS):
            img = image(D, kind)
            assert crc(img) == int(g["inputs_crc"][di, ki])
            for op in range(R.N_OPS):
                for b in range(R.N_BINS):
                    for neg in range(2):
                        assert crc(R.apply(img, R.row(op, b, neg, D))) == int(g["crc"][di, ki, op, b, neg]), (D, kind, R.OPS[op], b, neg)
    assert len(g["full"]) >= 12
    for j, (D, kind, op, b, neg) in enumerate(g["full"]):
        D, op, b, neg = int(D), int(op), int(b), int(neg)
        assert np.array_equal(g["full%02d" % j], R.apply(image(D, str(kind)), R.row(op, b, neg, D))), (D, kind, op, b, neg)


# ---- the record and the plan of the library ----
def c_row(lib, op, b, neg, D):
    from resnet_amd import binding as B
    r = B.MiTaRow()
    rc = lib.mi_ta_row(op, b, neg, D, C.byref(r))
    return rc, r.as_dict()


def _same_row(got, want):
    return (got["op"] == want["op"] and got["bin"] == want["bin"] and got["neg"] == want["neg"] and got["arg"] == want["arg"]
            and got["A"] == want["A"] and np.float32(got["factor"]).view(np.uint32) == np.float32(want["factor"]).view(np.uint32)
            and np.float64(got["magnitude"]).view(np.uint64) == np.float64(want["magnitude"]).view(np.uint64))


@pytest.mark.parametrize("D", [1, 7, 8, 30, 33, 224, 225, 4096])
def test_row_equals_the_python_row(lib, D):
    """every field, bit for bit (the sign of a zero magnitude included), every op x bin x sign"""
    for op in range(R.N_OPS):
        for b in range(R.N_BINS):
            for neg in range(2):
                rc, got = c_row(lib, op, b, neg, D)
                assert rc == 0 and _same_row(got, R.row(op, b, neg, D)), (R.OPS[op], b, neg, got, R.row(op, b, neg, D))


def test_struct_layout(lib):
    from resnet_amd import binding as B
    assert C.sizeof(B.MiTaRow) == 56 and B.MiTaRow.magnitude.offset == 16 and B.MiTaRow.factor.offset == 24 and B.MiTaRow.A.offset == 28
    geo = (C.c_size_t * 4)()
    lib.mi_debug_ta_geometry(geo)  # host only
    assert geo[0] == 256 and geo[1] >= 1 and geo[2] >= 1 and geo[3] == 4
    assert lib.mi_ta_workspace_bytes(5, 33) == 5 * 4096 + (5 * 3 * 33 * 33 + 15) // 16 * 16


def test_gather_sums_stay_below_2_31():
    """DESIGN.md "Size limits": at dim = 4096 no partial sum of A2 + A1 y + A0 x (or the y row) leaves int32, for every record"""
    for D in (4096, 4095):
        for op in R.GEOMETRIC:
            for b in range(R.N_BINS):
                for neg in range(2):
                    A = R.row(op, b, neg, D)["A"]
                    for base, cy, cx in ((A[2], A[1], A[0]), (A[5], A[4], A[3])):
                        for y in (0, D - 1):
                            for x in (0, D - 1):
                                assert all(abs(v) < 2 ** 31 for v in (base, cy * y, cx * x, base + cy * y, base + cy * y + cx * x))


def test_magnitude_tables_equal_torch_linspace():
    """the committed constants are torchvision's _augmentation_space(31): float32 torch.linspace widened to double"""
    import torch
    assert R.MAG_099 == [float(v) for v in torch.linspace(0.0, 0.99, 31)]
    assert R.MAG_32 == [float(v) for v in torch.linspace(0.0, 32.0, 31)]
    assert [R.magnitude(R.ROTATE, b) for b in range(31)] == [float(v) for v in torch.linspace(0.0, 135.0, 31)]
    assert [R.magnitude(R.SOLARIZE, b) for b in range(31)] == [float(v) for v in torch.linspace(255.0, 0.0, 31)]
    assert [R.magnitude(R.POSTERIZE, b) for b in range(31)] == [float(v) for v in 8 - (torch.arange(31) / ((31 - 1) / 6)).round().int()]
    assert [int(v) for v in R.MAG_32] == list(range(16)) + list(range(17, 31)) + [32]  # not bin 32 / 30


def test_library_tables_equal_the_committed_ones(lib):
    for op, table in ((R.SHEAR_X, R.MAG_099), (R.BRIGHTNESS, R.MAG_099), (R.TRANSLATE_Y, R.MAG_32)):
        assert [c_row(lib, op, b, 0, 32)[1]["magnitude"] for b in range(31)] == table


def test_quantise_inverts_decode_on_every_table_value():
    b = np.broadcast_to(np.arange(256, dtype=np.uint8).reshape(1, 1, 256), (3, 1, 256))
    v = R.decode(b)
    assert v.dtype == np.float32 and np.array_equal(R.quantise(v), b)
    # the R plane carries 103.94: plane d holds source position 2 - d
    assert v[0, 0, 0] == np.float32(-103.94) and v[2, 0, 255] == np.float32(255 - 123.68)


def test_quantise_rounds_other_values_as_a_conversion_to_bytes_would():
    v = np.zeros((3, 1, 8), np.float32)
    v[0, 0] = np.array([np.nan, np.inf, -np.inf, -500.0, 500.0, 0.5, 1.5, 2.4999], np.float32) - R.mean_plane(0)
    q = R.quantise(v)[0, 0]
    assert list(q[:5]) == [0, 255, 0, 0, 255] and all(abs(int(a) - b) <= 1 for a, b in zip(q[5:], (0, 2, 2)))


def c_plan(lib, seed, epoch, step, rank, world, n, D):
    from resnet_amd import binding as B
    rows = (B.MiTaRow * max(n, 1))()
    rc = lib.mi_ta_plan(seed & M64, epoch, step, rank, world, n, D, rows)
    return rc, [rows[i].as_dict() for i in range(n)]


def test_plan_equals_the_python_plan(lib):
    for seed in (0, 1, 2 ** 63 + 5):
        for epoch, step, rank, world in ((0, 0, 0, 1), (3, -1, 0, 1), (1, 40, 1, 4), (7, 2 ** 33, 3, 8)):
            for D in (30, 224):
                rc, got = c_plan(lib, seed, epoch, step, rank, world, 64, D)
                want = R.plan(seed, epoch, step % 2 ** 64, rank, world, 64, D)
                assert rc == 0 and all(_same_row(g, w) for g, w in zip(got, want)), (seed, epoch, step)


def test_plan_is_a_pure_function_of_its_arguments(lib):
    key = lambda rows: [(r["op"], r["bin"], r["neg"]) for r in rows]
    first = key(c_plan(lib, 5, 2, 40, 1, 4, 64, 32)[1])
    assert first == key(c_plan(lib, 5, 2, 40, 1, 4, 64, 32)[1])
    for other in ((6, 2, 40, 1, 4), (5, 3, 40, 1, 4), (5, 2, 41, 1, 4), (5, 2, 40, 2, 4)):
        assert key(c_plan(lib, *other, 64, 32)[1]) != first
    assert key(c_plan(lib, 5, 2, 10, 1, 4, 64, 32)[1]) == key(c_plan(lib, 5, 2, 41, 0, 1, 64, 32)[1])  # step world + rank
    assert key(c_plan(lib, 5, 2, 40, 1, 4, 8, 32)[1]) == first[:8]  # a row's draw does not depend on n


def test_op_bin_and_sign_are_uniform(lib):
    """6000 rows: each count within 5 binomial standard deviations of N / k"""
    N = 6000
    rows = c_plan(lib, 11, 0, 3, 0, 1, N, 224)[1]
    ki = [splitmix64_at(splitmix64_at(splitmix64_at(splitmix64_at(splitmix64_at(11, 0), 3), R.STEP_INDEX), i), 2) >> 63 for i in range(N)]
    for name, vals, k in (("op", [r["op"] for r in rows], 14), ("bin", [r["bin"] for r in rows], 31), ("neg", ki, 2)):
        counts = np.bincount(np.array(vals), minlength=k)
        sd = math.sqrt(N * (1 / k) * (1 - 1 / k))
        print(name, counts.tolist(), "expected %.1f, standard deviation %.1f" % (N / k, sd))
        assert len(counts) == k and np.all(np.abs(counts - N / k) <= 5 * sd), name
    # the stored sign is the draw on the signed operations and 0 on the others
    assert all(r["neg"] == (s if r["op"] in R.SIGNED else 0) for r, s in zip(rows, ki))


def test_equal_seeds_share_no_draw_with_the_erase_and_mix_plans():
    """the three plans hang under one step key k: mix draws splitmix64_at(k, 0 .. 131), erase under splitmix64_at(k, 1000), this plan under
    splitmix64_at(k, 2000).  No value of one plan's stream occurs in another's"""
    for seed, epoch, step, rank, world in ((0, 0, 0, 0, 1), (7, 3, 12, 1, 2)):
        k = splitmix64_at(splitmix64_at(seed, epoch), step * world + rank)
        mix = {splitmix64_at(k, j) for j in range(200)}
        e = eraseref.step_key(seed, epoch, step, rank, world)
        a = splitmix64_at(k, R.STEP_INDEX)
        assert e == splitmix64_at(k, eraseref.STEP_INDEX) and a != e and a not in mix and e not in mix
        erase = {splitmix64_at(splitmix64_at(e, i), j) for i in range(64) for j in range(41)} | {splitmix64_at(e, i) for i in range(64)}
        ta = {splitmix64_at(splitmix64_at(a, i), j) for i in range(64) for j in range(3)} | {splitmix64_at(a, i) for i in range(64)}
        assert len(ta) == 64 * 4 and not (ta & erase) and not (ta & mix)


@pytest.mark.parametrize("args,word", [((14, 0, 0, 32), "op"), ((-1, 0, 0, 32), "op"), ((1, 31, 0, 32), "bin"), ((1, -1, 0, 32), "bin"),
                                       ((1, 0, 2, 32), "neg"), ((1, 0, 0, 0), "dim"), ((1, 0, 0, 4097), "dim")])
def test_row_refusals(lib, args, word):
    rc, _ = c_row(lib, *args)
    msg = lib.mi_last_error().decode()
    lib.mi_clear_error()
    assert rc == -1 and "mi_ta_row" in msg and word in msg, msg
    from resnet_amd import binding as B
    assert lib.mi_ta_row(1, 0, 0, 32, None) == -1
    lib.mi_clear_error()


@pytest.mark.parametrize("kw,word", [(dict(n=-1), "n"), (dict(dim=0), "dim"), (dict(dim=4097), "dim"), (dict(rank=1), "rank"),
                                     (dict(rank=-1), "rank"), (dict(world=0), "rank")])
def test_plan_refusals(lib, kw, word):
    a = dict(rank=0, world=1, n=4, dim=32)
    a.update(kw)
    rc, _ = c_plan(lib, 1, 0, 0, a["rank"], a["world"], a["n"], a["dim"])
    msg = lib.mi_last_error().decode()
    lib.mi_clear_error()
    assert rc == -1 and "mi_ta_plan" in msg and word in msg, msg
    assert lib.mi_ta_plan(1, 0, 0, 0, 1, 4, 32, None) == -1  # rows without a place to put them
    lib.mi_clear_error()
    assert lib.mi_ta_plan(1, 0, 0, 0, 1, 0, 32, None) == 0   # no rows: nothing to write
