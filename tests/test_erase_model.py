"""mi_erase_plan against its Python restatement (tests/eraseref.py) bit for bit, the plan's rules and distribution, its refusals, and the
noise model on its own: moments over 10^6 elements and what a value depends on.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import eraseref as R

SCALE, RATIO = (0.02, 0.33), (0.3, 3.3)
N_ROWS = 20000
STAT_SEED = 20261020


@pytest.fixture(scope="module")
def lib():
    from resnet_amd import binding
    return binding.load()


def c_plan(lib, seed, epoch, step, rank, world, n, dim, prob, scale=SCALE, ratio=RATIO):
    out = np.full((max(n, 1), 4), -7, np.int32)
    rc = lib.mi_erase_plan(seed, epoch, step, rank, world, n, dim, prob, scale[0], scale[1], ratio[0], ratio[1], out.ctypes.data)
    if rc != 0:
        msg = lib.mi_last_error().decode()
        lib.mi_clear_error()
        return rc, msg
    return 0, out[:max(n, 0)]


@pytest.mark.parametrize("dim", [1, 2, 7, 32, 224])
def test_plan_equals_the_python_plan(lib, dim):
    """bit for bit over seeds x epochs x steps x ranks (step -1 is the trainer's first), n = 64, at prob 1, 0.5 and two scale ranges"""
    boxed = 0
    for seed in (0, 1, 2 ** 63 + 5):
        for epoch in (0, 3):
            for step in (-1, 0, 17, 2 ** 31):
                for rank, world in ((0, 1), (1, 4), (3, 4)):
                    for prob, scale in ((1.0, SCALE), (0.5, SCALE), (1.0, (0.3, 1.2))):
                        rc, got = c_plan(lib, seed, epoch, step, rank, world, 64, dim, prob, scale)
                        want = R.plan(seed, epoch, step, rank, world, 64, dim, prob, scale, RATIO)
                        assert rc == 0 and np.array_equal(got, want), (seed, epoch, step, rank, world, prob, scale)
                        boxed += int(np.sum((got[:, 2] > 0) & (got[:, 3] > 0)))
    assert boxed > 0 or dim == 1  # D = 1: h < 1 leaves only the empty box


@pytest.mark.parametrize("dim", [1, 2, 7, 32, 224])
def test_prob_0_and_1_and_the_box_rules(lib, dim):
    rc, none = c_plan(lib, 3, 1, 5, 0, 1, 64, dim, 0.0)
    assert rc == 0 and not none.any()
    rc, got = c_plan(lib, 3, 1, 5, 0, 1, 64, dim, 1.0)
    want, drawn, taken = R.plan_rows(3, 1, 5, 0, 1, 64, dim, 1.0, SCALE, RATIO)
    assert rc == 0 and np.array_equal(got, want)
    assert drawn.all()  # prob 1: a draw for every row
    y0, x0, h, w = got.T
    assert np.all((h >= 0) & (h < dim) & (w >= 0) & (w < dim))  # strict, as torchvision
    assert np.all((y0 >= 0) & (y0 + h <= dim) & (x0 >= 0) & (x0 + w <= dim))
    assert not got[~taken].any()
    if dim >= 32:
        assert np.all(taken) and np.all((h > 0) & (w > 0))


@pytest.mark.parametrize("dim", [2, 7, 224])
def test_scale_1_never_yields_a_box(lib, dim):
    """target = D^2: h w = D^2 needs a side >= D, every try fails, the row falls through as torchvision's image does"""
    rc, got = c_plan(lib, 11, 0, 0, 0, 1, 64, dim, 1.0, (1.0, 1.0))
    want, drawn, taken = R.plan_rows(11, 0, 0, 0, 1, 64, dim, 1.0, (1.0, 1.0), RATIO)
    assert rc == 0 and not got.any() and drawn.all() and not taken.any() and not want.any()


def test_plan_is_a_pure_function_of_its_arguments(lib):
    base = dict(seed=5, epoch=2, step=40, rank=1, world=4)
    args = lambda d: (d["seed"], d["epoch"], d["step"], d["rank"], d["world"], 64, 32, 1.0)
    first = c_plan(lib, *args(base))[1]
    assert np.array_equal(first, c_plan(lib, *args(base))[1])
    for key, other in (("seed", 6), ("epoch", 3), ("step", 41), ("rank", 2)):
        assert not np.array_equal(c_plan(lib, *args(dict(base, **{key: other})))[1], first), key
    # ranks of one step and the steps of one rank never share an index: step world + rank
    assert np.array_equal(c_plan(lib, 5, 2, 10, 1, 4, 64, 32, 1.0)[1], c_plan(lib, 5, 2, 41, 0, 1, 64, 32, 1.0)[1])
    # a row's draw does not depend on n
    assert np.array_equal(c_plan(lib, 5, 2, 40, 1, 4, 8, 32, 1.0)[1], first[:8])
    assert c_plan(lib, 5, 2, 40, 1, 4, 0, 32, 1.0)[0] == 0


def test_erased_share_and_box_areas(lib):
    """D = 224, prob = 0.1, 20 000 rows.  The erased share lies within 5 binomial standard deviations of 0.1.  Every taken box's area:
    h = round(fh) and w = round(fw) lie within 0.5 of fh and fw with fh fw = target in [lo, hi] D^2, so
    h w >= (fh - 0.5) (fw - 0.5) = target - (fh + fw) / 2 + 0.25 and h w <= target + (fh + fw) / 2 + 0.25, and fh + fw <= h + w + 1:
    lo D^2 - (h + w + 1) / 2 <= h w <= hi D^2 + (h + w + 1) / 2 + 0.25 (a relative 10^-12 for the roundings of the doubles)"""
    D, prob = 224, 0.1
    rc, got = c_plan(lib, STAT_SEED, 0, 0, 0, 1, N_ROWS, D, prob)
    assert rc == 0 and np.array_equal(got, R.plan(STAT_SEED, 0, 0, 0, 1, N_ROWS, D, prob, SCALE, RATIO))
    y0, x0, h, w = got.astype(np.int64).T
    erased = (h > 0) & (w > 0)
    share, sd = erased.mean(), math.sqrt(prob * (1 - prob) / N_ROWS)
    print("erased share %.5f of %d rows (expected %.2f, standard deviation %.5f)" % (share, N_ROWS, prob, sd))
    assert abs(share - prob) <= 5 * sd
    area, slack = (h * w)[erased], (h + w + 1)[erased] / 2.0
    lo, hi = SCALE[0] * D * D * (1 - 1e-12), SCALE[1] * D * D * (1 + 1e-12)
    print("h w / D^2 of the taken boxes: %.5f .. %.5f" % (area.min() / D ** 2, area.max() / D ** 2))
    assert np.all(area >= lo - slack) and np.all(area <= hi + slack + 0.25)
    assert np.all((h < D) & (w < D) & (y0 + h <= D) & (x0 + w <= D))
    assert not got[~erased].any()


@pytest.mark.parametrize("kw,word", [
    (dict(n=-1), "n >= 0"), (dict(dim=0), "dim"), (dict(dim=16385), "dim"), (dict(prob=-0.1), "prob"), (dict(prob=1.5), "prob"),
    (dict(prob=float("nan")), "prob"), (dict(scale=(0.0, 0.3)), "scale_lo"), (dict(scale=(-0.1, 0.3)), "scale_lo"), (dict(scale=(0.3, 0.2)), "scale_hi"),
    (dict(ratio=(0.0, 3.3)), "ratio_lo"), (dict(ratio=(2.0, 1.0)), "ratio_hi"), (dict(scale=(float("nan"), 0.3)), "scale_lo"),
    (dict(rank=1, world=1), "rank"), (dict(rank=-1, world=2), "rank"), (dict(rank=0, world=0), "rank")])
def test_refusals(lib, kw, word):
    a = dict(rank=0, world=1, n=4, dim=32, prob=0.5, scale=SCALE, ratio=RATIO)
    a.update(kw)
    rc, msg = c_plan(lib, 1, 0, 0, a["rank"], a["world"], a["n"], a["dim"], a["prob"], a["scale"], a["ratio"])
    assert rc == -1 and "mi_erase_plan" in msg and word in msg, msg


def test_a_huge_scale_is_no_error(lib):
    """target overflows every side: no try is taken, nothing is converted out of range"""
    rc, got = c_plan(lib, 1, 0, 0, 0, 1, 16, 32, 1.0, (1e300, 1e308))
    assert rc == 0 and not got.any()
    assert not R.plan(1, 0, 0, 0, 1, 16, 32, 1.0, (1e300, 1e308), RATIO).any()


# ---------------------------------------------------------------- the noise model
def test_noise_moments():
    """10^6 elements: the mean of N values of variance ~1 has standard error 1 / sqrt(N); the sample variance of a sum of twelve uniforms
    (excess kurtosis -1.2 / 12 = -0.1) has standard error sqrt((mu4 - var^2) / N) = sqrt((3 - 0.1 - 1) / N) = sqrt(1.9 / N)"""
    N = 10 ** 6
    z = R.noise_at(12345, 3, np.arange(N)).astype(np.float64)
    mean, var = z.mean(), z.var()
    print("noise over %d elements: mean %.6f (5 se %.6f), variance %.6f (5 se %.6f), |z| max %.4f" % (N, mean, 5 / math.sqrt(N), var, 5 * math.sqrt(1.9 / N), np.abs(z).max()))
    assert abs(mean) <= 5 / math.sqrt(N)
    assert abs(var - 1.0) <= 5 * math.sqrt(1.9 / N)
    assert np.abs(z).max() < 6.0


def test_a_noise_value_depends_on_seed_row_and_position_only():
    D = 9
    full = R.noise(7, 2, D)
    c, y, x = 1, 4, 6
    assert full[c, y, x] == R.noise_at(7, 2, np.array([(c * D + y) * D + x]))[0]
    x0 = np.zeros((4, 3, D, D), np.float32)
    a = R.erase(x0, [(0, 0, D, D)] * 4, "noise", noise_seed=7)
    b = R.erase(x0, [(2, 3, 4, 5)] * 4, "noise", noise_seed=7)
    assert np.array_equal(a[:, :, 2:6, 3:8], b[:, :, 2:6, 3:8]) and np.array_equal(a[2], full)  # value 0, std 1: z itself
    assert np.array_equal(R.erase(x0[:1], [(0, 0, D, D)], "noise", noise_seed=7, first_row=2)[0], full)
    for other in (R.noise(8, 2, D), R.noise(7, 3, D)):
        assert np.mean(other != full) > 0.99
    assert len(np.unique(full)) > 0.9 * full.size  # positions differ
    # the scalar definition, on Python ints
    q = R.splitmix64_at(7, 2)
    el = (c * D + y) * D + x
    S = sum((R.splitmix64_at(q, 64 + 3 * el + m) >> (16 * f)) & 0xFFFF for m in range(3) for f in range(4))
    assert full[c, y, x] == np.float32((S - 393210) / 65536.0)


def test_erase_model_keeps_everything_outside_the_boxes():
    x = np.arange(3 * 3 * 5 * 5, dtype=np.float32).reshape(3, 3, 5, 5)
    x[1, 0, 0, 0] = np.float32(-0.0)
    got = R.erase(x, [(0, 0, 0, 0), (1, 2, 2, 9), (-3, -1, 2, 2)], "const", value=(1, 2, 3))
    assert np.array_equal(got[0].view(np.uint32), x[0].view(np.uint32))
    keep = np.ones((5, 5), bool)
    keep[1:3, 2:] = False
    assert np.array_equal(got[1][:, keep].view(np.uint32), x[1][:, keep].view(np.uint32))
    assert all(np.all(got[1, c, 1:3, 2:] == c + 1) for c in range(3))
    assert np.all(got[2, :, :2, :2] == np.array([1, 2, 3], np.float32)[:, None, None])  # a negative origin is clamped to 0, the size kept


def test_library_exports_the_erase_entry_points(lib):
    from resnet_amd import binding
    for name in ("mi_erase_plan", "mi_op_erase_batch", "mi_debug_erase_geometry", "mi_trainer_set_erase", "mi_trainer_last_erase"):
        assert hasattr(lib, name) and name in binding.PROTOTYPES, name
    assert C.sizeof(binding.MiEraseFill) == 40 and binding.MiEraseFill.noise_seed.offset == 32
    geo = (C.c_size_t * 4)()
    lib.mi_debug_erase_geometry(geo)  # host only
    assert geo[0] % 64 == 0 and geo[2] == geo[0] // 64 and geo[1] >= 1 and geo[3] == 256
