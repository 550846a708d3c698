"""mi_mix_plan against its Python restatement (tests/mixref.py) field for field, the plan's distribution against Beta(alpha, alpha) and the
settings' probabilities, its refusals, and the derived row-loss bound of the two-label head against a float32 restatement of the kernel's
steps.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import lossref
import mixref as R

N_DRAWS = 20000
STAT_SEED = 20261019


@pytest.fixture(scope="module")
def lib():
    from resnet_amd import binding
    return binding.load()


def c_plan(lib, seed, epoch, step, rank, world, ma, ca, prob, switch, dim):
    from resnet_amd import binding as B
    p = B.MiMixPlan()
    rc = lib.mi_mix_plan(seed, epoch, step, rank, world, ma, ca, prob, switch, dim, C.byref(p))
    if rc != 0:
        msg = lib.mi_last_error().decode()
        lib.mi_clear_error()
        return rc, msg
    return 0, p.as_dict()


def same_plan(got, want):
    return all(got[k] == want[k] for k in ("mode", "y0", "x0", "y1", "x1")) and np.float32(got["lam"]).tobytes() == np.float32(want["lam"]).tobytes()


@pytest.mark.parametrize("dim", [7, 32, 224])
@pytest.mark.parametrize("alpha", [0.2, 0.8, 1.0])
def test_plan_equals_the_python_plan(lib, alpha, dim):
    """field for field, lam bit for bit, over seeds x epochs x steps x ranks (step -1 is the trainer's first) and the three ways to
    choose a mode, with and without mode-0 draws"""
    settings = [(alpha, 0.0, 1.0, 0.5), (0.0, alpha, 1.0, 0.5), (alpha, alpha, 1.0, 0.5), (alpha, 1.0, 0.5, 0.3)]
    modes = set()
    for seed in (0, 1, 2 ** 63 + 5):
        for epoch in (0, 3):
            for step in (-1, 0, 1, 17, 2 ** 31):
                for rank, world in ((0, 1), (1, 4), (3, 4)):
                    for ma, ca, prob, switch in settings:
                        rc, got = c_plan(lib, seed, epoch, step, rank, world, ma, ca, prob, switch, dim)
                        want = R.plan(seed, epoch, step, rank, world, ma, ca, prob, switch, dim)
                        assert rc == 0 and same_plan(got, want), ((seed, epoch, step, rank, world, ma, ca, prob, switch), got, want)
                        modes.add(got["mode"])
    assert modes == {0, 1, 2}


def test_plan_is_a_pure_function_of_its_arguments(lib):
    base = dict(seed=5, epoch=2, step=40, rank=1, world=4)
    args = lambda d: (d["seed"], d["epoch"], d["step"], d["rank"], d["world"], 0.8, 0.0, 1.0, 0.5, 32)
    first = c_plan(lib, *args(base))[1]
    assert first == c_plan(lib, *args(base))[1] and first["mode"] == 1
    for key, other in (("seed", 6), ("epoch", 3), ("step", 41), ("rank", 2)):
        moved = c_plan(lib, *args(dict(base, **{key: other})))[1]
        assert moved["lam"] != first["lam"], key
    # ranks of one step and the steps of one rank never share an index: step world + rank
    assert c_plan(lib, 5, 2, 10, 1, 4, 0.8, 0.0, 1.0, 0.5, 32)[1] == c_plan(lib, 5, 2, 41, 0, 1, 0.8, 0.0, 1.0, 0.5, 32)[1]


def _draws(lib, ma, ca, prob, switch, dim=32, seed=STAT_SEED):
    return [c_plan(lib, seed, 0, step, 0, 1, ma, ca, prob, switch, dim)[1] for step in range(N_DRAWS)]


def test_mode_fractions(lib):
    """prob 0.5: mode 0 in half of the draws; switch 0.5: CutMix in half of the rest; each within 5 standard errors of a binomial share"""
    d = _draws(lib, 0.2, 1.0, 0.5, 0.5)
    none = sum(p["mode"] == 0 for p in d)
    se = math.sqrt(0.5 * 0.5 / N_DRAWS)
    print("mode 0: %.4f of %d draws (expected 0.5, standard error %.4f)" % (none / N_DRAWS, N_DRAWS, se))
    assert abs(none / N_DRAWS - 0.5) <= 5 * se
    mixed = N_DRAWS - none
    cut = sum(p["mode"] == 2 for p in d)
    se = math.sqrt(0.5 * 0.5 / mixed)
    print("CutMix: %.4f of %d mixed draws (expected 0.5, standard error %.4f)" % (cut / mixed, mixed, se))
    assert abs(cut / mixed - 0.5) <= 5 * se
    assert all(p["lam"] == 1.0 and (p["y0"], p["x0"], p["y1"], p["x1"]) == (0, 0, 0, 0) for p in d if p["mode"] == 0)


@pytest.mark.parametrize("alpha", [0.2, 0.8, 1.0])
def test_lambda_is_beta_distributed(lib, alpha):
    """mean 1/2 and variance 1 / (4 (2 alpha + 1)) of Beta(alpha, alpha) over 20 000 mixup draws, each within 5 standard errors: of the mean
    sqrt(var / n); of the variance sqrt((mu4 - var^2) / n) with the fourth central moment mu4 = var^2 (3 - 6 / (2 alpha + 3)), the symmetric
    Beta's excess kurtosis being -6 / (2 alpha + 3)"""
    lam = np.array([p["lam"] for p in _draws(lib, alpha, 0.0, 1.0, 0.5)], np.float64)
    assert np.all((lam >= 0) & (lam <= 1))
    var = 1.0 / (4.0 * (2.0 * alpha + 1.0))
    se_mean = math.sqrt(var / N_DRAWS)
    se_var = var * math.sqrt((2.0 - 6.0 / (2.0 * alpha + 3.0)) / N_DRAWS)
    got_var = float(np.mean((lam - 0.5) ** 2))
    print("alpha %g: mean %.5f (0.5 +- %.5f), variance %.5f (%.5f +- %.5f)" % (alpha, lam.mean(), se_mean, got_var, var, se_var))
    assert abs(lam.mean() - 0.5) <= 5 * se_mean
    assert abs(got_var - var) <= 5 * se_var


def test_johnk_fallback_is_rare(lib):
    """at alpha = 1 a try is taken with probability 1/2, 64 tries fail with 2^-64: at most 1 draw in 20 000 may end in the fallback.  The
    Python plan counts them for the seed the statistics use; the library's plans equal the Python ones on all of those draws"""
    ref = [R.plan(STAT_SEED, 0, step, 0, 1, 1.0, 0.0, 1.0, 0.5, 32) for step in range(N_DRAWS)]
    assert sum(p["fallback"] for p in ref) <= 1
    got = _draws(lib, 1.0, 0.0, 1.0, 0.5)
    assert all(same_plan(g, w) for g, w in zip(got, ref))


@pytest.mark.parametrize("dim", [7, 32, 224])
def test_cutmix_boxes_lie_inside_the_image(lib, dim):
    seen_clamped = False
    for step in range(2000):
        p = c_plan(lib, 9, 1, step, 0, 1, 0.0, 1.0, 1.0, 0.5, dim)[1]
        assert p["mode"] == 2
        assert 0 <= p["y0"] <= p["y1"] <= dim and 0 <= p["x0"] <= p["x1"] <= dim, p
        area = (p["y1"] - p["y0"]) * (p["x1"] - p["x0"])
        assert np.float32(p["lam"]).tobytes() == np.float32(1.0 - area / (dim * dim)).tobytes()
        seen_clamped |= p["y0"] == 0 or p["x0"] == 0 or p["y1"] == dim or p["x1"] == dim
    assert seen_clamped


@pytest.mark.parametrize("args,word", [
    ((0.0, 0.0, 1.0, 0.5, 32), "both alphas"), ((-0.2, 0.0, 1.0, 0.5, 32), "alpha"), ((0.0, -1.0, 1.0, 0.5, 32), "alpha"),
    ((1.5, 0.0, 1.0, 0.5, 32), "alpha"), ((0.2, 1.0001, 1.0, 0.5, 32), "alpha"), ((float("nan"), 1.0, 1.0, 0.5, 32), "alpha"),
    ((0.2, 1.0, -0.1, 0.5, 32), "prob"), ((0.2, 1.0, 1.1, 0.5, 32), "prob"), ((0.2, 1.0, 1.0, -0.5, 32), "switch_prob"),
    ((0.2, 1.0, 1.0, 1.5, 32), "switch_prob"), ((0.2, 1.0, 1.0, 0.5, 0), "dim"), ((0.2, 1.0, 1.0, 0.5, -3), "dim")])
def test_refusals(lib, args, word):
    rc, msg = c_plan(lib, 1, 0, 0, 0, 1, *args)
    assert rc == -1 and "mi_mix_plan" in msg and word in msg, msg


def test_refuses_a_rank_outside_the_world(lib):
    for rank, world in ((1, 1), (-1, 2), (0, 0)):
        rc, msg = c_plan(lib, 1, 0, 0, rank, world, 0.2, 1.0, 1.0, 0.5, 32)
        assert rc == -1 and "rank" in msg


def test_mix_model_pairs_rows_from_both_ends():
    x = np.arange(5 * 3 * 4 * 4, dtype=np.float32).reshape(5, 3, 4, 4)
    half = R.mix(x, dict(mode=1, lam=np.float32(0.5), y0=0, x0=0, y1=0, x1=0))
    assert np.array_equal(half[0], half[4]) and np.array_equal(half[1], half[3]) and np.array_equal(half[2], x[2])
    assert np.array_equal(half[0], (x[0] + x[4]) / 2)
    cut = R.mix(x, dict(mode=2, lam=np.float32(0.75), y0=1, x0=2, y1=3, x1=9))
    assert np.array_equal(cut[0, :, 1:3, 2:], x[4, :, 1:3, 2:]) and np.array_equal(cut[4, :, 1:3, 2:], x[0, :, 1:3, 2:])
    keep = np.ones((4, 4), bool)
    keep[1:3, 2:] = False
    assert np.array_equal(cut[:, :, keep], x[:, :, keep]) and np.array_equal(cut[2], x[2])


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("shape", lossref.SHAPES)
def test_two_label_model_is_the_weighted_sum_of_one_label_heads(shape, eps):
    """the float64 two-label head: loss and gradient are lam x (label a) + (1 - lam) x (label b) of lossref.loss_head, and lam = 1 is it"""
    x, a = lossref.make_inputs(*shape)
    b = R.labels_b(a)
    pa, da, la, ra = lossref.loss_head(x, a, eps)
    _, db, lb, _ = lossref.loss_head(x, b, eps)
    for lam in (0.0, 0.25, 1.0):
        pred, dl, loss, rank = R.loss_head_mix(x, a, b, lam, eps)
        assert np.array_equal(pred, pa) and np.array_equal(rank, ra)
        assert np.max(np.abs(dl - (lam * da + (1 - lam) * db))) <= 1e-15
        want = lam * la + (1 - lam) * lb
        assert np.max(np.abs(loss - want) / (1.0 + want)) <= 1e-13
    assert np.array_equal(R.loss_head_mix(x, a, b, 1.0, eps)[1], da)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("lam", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("shape", lossref.SHAPES)
def test_fp32_two_label_formulas_stay_inside_the_derived_bound(shape, lam, eps):
    """DESIGN.md, "Loss head": the second label's term adds one subtraction and the roundings of wb z_b; the per-row bound stays
    2^-19 (2 + ref) against the two-label float64 value.  b = the partner's label (a != b in most rows) and b = a"""
    x, a = lossref.make_inputs(*shape)
    for b in (R.labels_b(a), a):
        ref = R.loss_head_mix(x, a, b, np.float32(lam), eps)[2]
        got = R.loss_head_mix_f32(x, a, b, lam, eps).astype(np.float64)
        share = np.max(np.abs(got - ref) / lossref.loss_bound(ref))
        print("fp32 two-label formulas, %s lam %g eps %g: worst |error| / bound = %.4f" % (shape, lam, eps, share))
        assert np.all(np.isfinite(got)) and share <= 1.0


def test_f32_targets_at_lam_one_are_the_one_label_targets():
    f = np.float32
    a, b = np.array([3, 0, 9]), np.array([5, 77, -1])
    for eps in (0.0, 0.1):
        t = R.targets_f32(10, a, b, 1.0, eps)
        u = f(eps) / f(10)
        want = np.full((3, 10), u, f)
        want[np.arange(3), a] = (f(1) - f(eps)) + u
        assert np.array_equal(t.view(np.uint32), want.view(np.uint32))


def test_the_inputs_of_the_rounding_mutants_separate_them():
    """the mutant table's pre-check (tests/mutants.py, loss_mix_wb_as_difference and loss_mix_target_sum_reassociated): the operator
    cases named as their killers see other float32 targets under the fault.  wb: not at the operator tests' lam = 0.3, but at WB_LAM,
    WB_EPS.  The association: only with a == b, and of lossref.SHAPES at eps 0.1, lam 0.3 only where L = 65"""
    f = np.float32
    for eps in (0.0, 0.1):
        assert R.wb_as_difference(0.3, eps) == (f(1) - f(eps)) * (f(1) - f(0.3)), "lam = 0.3 has begun to separate: name it as a killer"
    wb = (f(1) - f(R.WB_EPS)) * (f(1) - f(R.WB_LAM))
    assert R.wb_as_difference(R.WB_LAM, R.WB_EPS) in (np.nextafter(wb, f(0)), np.nextafter(wb, f(1)))
    seen = {}
    for shape in lossref.SHAPES:
        _, a = lossref.make_inputs(*shape)
        b = R.labels_b(a)
        assert np.array_equal(R.targets_f32(shape[1], a, b, 0.3, 0.1)[a != b], R.targets_reassociated_f32(shape[1], a, b, 0.3, 0.1)[a != b])
        t, t2 = R.targets_f32(shape[1], a, a, 0.3, 0.1), R.targets_reassociated_f32(shape[1], a, a, 0.3, 0.1)
        seen[shape] = int(np.sum(np.any(t != t2, axis=1)))
    assert seen[(4, 65)] == 4 and sum(seen.values()) == 4, seen


def test_library_exports_the_mix_entry_points(lib):
    from resnet_amd import binding
    for name in ("mi_mix_plan", "mi_op_mix_batch", "mi_op_loss_head_mix", "mi_trainer_set_mix", "mi_trainer_last_mix", "mi_debug_mix_geometry"):
        assert hasattr(lib, name) and name in binding.PROTOTYPES, name
    assert C.sizeof(binding.MiMixPlan) == 24
    geo = (C.c_size_t * 3)()
    lib.mi_debug_mix_geometry(geo)  # host only
    assert geo[0] % 64 == 0 and geo[2] == geo[0] // 64 and geo[1] >= 1
