"""Weight averaging without a GPU: the model (tests/emaref.py) against torch.lerp, the library's host-only weight function against the
model, the exports, and the mutant table's uniqueness rule on the changed kernels_optim.hip."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import emaref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = [np.float32(1 - 0.9999), np.float32(0.1), np.float32(0.8), np.float32(1.0), np.float32(0.5)]
NEW_SYMBOLS = ["mi_ema_weight", "mi_op_ema_update", "mi_op_exchange", "mi_trainer_set_ema", "mi_trainer_ema_reset", "mi_trainer_ema_updates",
               "mi_trainer_eval_use_ema", "mi_trainer_ema_get_location", "mi_trainer_ema_set_location", "mi_trainer_ema_get_running_stats",
               "mi_trainer_ema_set_running_stats", "mi_debug_ema_geometry"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _inputs():
    rng = np.random.RandomState(0)
    e = (0.1 * rng.randn(1 << 20)).astype(np.float32)
    p = (e + 0.01 * rng.randn(1 << 20)).astype(np.float32)
    return e, p


def test_weight_function_equals_the_model_bit_for_bit():
    from resnet_amd import binding as B
    L = B.load()
    for decay in (0.0, 0.5, 0.9, 0.9999, 0.99998):
        for warmup in (0, 1):
            for k in list(range(41)) + [10 ** 3, 10 ** 6]:
                got, want = np.float32(L.mi_ema_weight(decay, warmup, k)), M.weight(decay, warmup, k)
                assert _bits(got) == _bits(want), (decay, warmup, k, got, want)
    # timm's warm-up: 0.1, 2 / 11, ... until the decay takes over; no warm-up: the decay from the first update
    assert M.weight(0.9999, True, 0) == np.float32(0.9) and M.weight(0.9999, True, 1) == np.float32(1 - 2 / 11)
    assert M.weight(0.9999, True, 10 ** 6) == M.weight(0.9999, False, 0) == np.float32(1 - 0.9999)


@pytest.mark.parametrize("w", WEIGHTS, ids=["%g" % w for w in WEIGHTS])
def test_lerp32_is_torch_lerp(w):
    """2^20 values (a multiple of 64: torch's vectorised body, whose bits the definition is; its scalar tail rounds differently)"""
    e, p = _inputs()
    want = torch.lerp(torch.from_numpy(e), torch.from_numpy(p), float(w)).numpy()
    got = M.lerp32(e, p, w)
    bad = int(np.sum(_bits(got) != _bits(want)))
    print("w = %r: %d of %d elements differ from torch.lerp" % (w, bad, e.size))
    assert bad == 0


def test_the_fma_is_part_of_the_definition():
    """the unfused e + w (p - e), every operation rounded, is not torch.lerp: the model must not degenerate into it"""
    e, p = _inputs()
    for w in WEIGHTS[:3]:
        unfused = (e + (w * (p - e)).astype(np.float32)).astype(np.float32) if w < 0.5 else \
            (p - ((p - e) * (np.float32(1) - w)).astype(np.float32)).astype(np.float32)
        assert int(np.sum(_bits(unfused) != _bits(M.lerp32(e, p, w)))) > 0


def test_fma32_is_exact_where_float64_rounds_twice():
    from fractions import Fraction
    # (1 + 2^-12)^2 - 2^-11 = 1 + 2^-24 exactly: a tie between two float32 values, half-even goes down to 1
    got = M.fma32(np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(-(2.0 ** -11)))  # = 1 + 2^-24: a tie, down to 1
    assert got == np.float32(1.0)
    # b one unit larger: the sum is 1 + 2^-24 + 2^-23 + 2^-35, just above a tie -- a float64 evaluation drops nothing here, but the check
    # against exact rational arithmetic below is what pins the rounding
    got = M.fma32(np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12 + 2.0 ** -23), np.float32(-(2.0 ** -11)))
    exact = Fraction(float(np.float32(1 + 2.0 ** -12))) * Fraction(float(np.float32(1 + 2.0 ** -12 + 2.0 ** -23))) - Fraction(2) ** -11
    lo = np.float32(float(exact))
    cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
    best = min(cands, key=lambda v: abs(Fraction(float(v)) - exact))
    assert got == best
    # random triples against exact rational arithmetic with a neighbour check
    rng = np.random.RandomState(5)
    a, b, c = (rng.randn(2000).astype(np.float32) for _ in range(3))
    c = (c * np.float32(1e-3)).astype(np.float32)
    got = M.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        g = got[i]
        err = abs(Fraction(float(g)) - exact)
        for nb in (np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))):
            assert err <= abs(Fraction(float(nb)) - exact), (i, a[i], b[i], c[i], g)


def test_exact_properties_and_the_non_finite_rule():
    e, p = _inputs()
    e = e.copy()
    e[:4] = [0.0, -0.0, 1.5, -2.25]
    for w in WEIGHTS:
        same = M.lerp32(e, e, w)
        assert np.array_equal(same, e), "p == e: the value stays"
        # fmaf(w, +0, -0) = +0: below 0.5 a -0 becomes +0; fmaf(-(1 - w), +0, -0) = -0 + -0: at and above 0.5 it stays -0, as in torch
        assert _bits(same)[1] == (0 if w < 0.5 else 0x80000000)
        assert np.array_equal(_bits(same)[2:], _bits(e)[2:])
    assert np.array_equal(_bits(M.lerp32(e, p, np.float32(1.0))), _bits(p)), "w == 1: p's bits"
    for w in WEIGHTS:
        pp, ee = p.copy(), e.copy()
        pp[[5, 6, 7]] = [np.inf, -np.inf, np.nan]
        ee[[9, 10, 11]] = [np.inf, -np.inf, np.nan]
        pp[12], ee[12] = np.float32(3e38), np.float32(-3e38)  # the difference overflows
        got, clean = M.lerp32(ee, pp, w), M.lerp32(e, p, w)
        for i in (5, 6, 7, 9, 10, 11, 12):
            assert _bits(got)[i] == _bits(ee)[i], (w, i)
        keep = np.ones(e.size, bool)
        keep[[5, 6, 7, 9, 10, 11, 12]] = False
        assert np.array_equal(_bits(got)[keep], _bits(clean)[keep])


def _kernel_lengths(vector):
    """the length set of tests/test_gpu_ema.py, from the launcher's own constants (host only)"""
    from resnet_amd import binding as B
    geo = (C.c_size_t * 4)()
    B.load().mi_debug_ema_geometry(geo)
    turn = int(geo[1] if vector else geo[2])
    return sorted({1, 3, 4, 5, 1023, 1024, 1025, turn - 1, turn, turn + 1}), turn


@pytest.mark.parametrize("w", [np.float32(0.1), np.float32(0.8), np.float32(0.5)], ids=["0.1", "0.8", "0.5"])
@pytest.mark.parametrize("vector", [True, False], ids=["vector", "element-wise"])
def test_separating_inputs_separate_every_tail_and_partial_turn_position(vector, w):
    """a condition, not a measurement: at every length of the operator test, every position of the n % 4 tail and of the partial turn
    (and every other one) tells the model from the alternative -- unfused at w = 0.1 and 0.8, the other branch at 0.5.  The operator
    test's older inputs do so in 2 to 6 % of the positions, and in none at n <= 5"""
    lengths, turn = _kernel_lengths(vector)
    covered = 0
    for n in lengths:
        e, p = M.separating_pair(n, w, n)
        assert e.size == p.size == n and e.dtype == p.dtype == np.float32
        differ = _bits(M.lerp32(e, p, w)) != _bits(M.alternative32(e, p, w))
        at = M.tail_and_partial_turn(n, turn, vector)
        assert at.any() or n % turn == 0
        assert differ[at].all() and differ.all(), "n = %d: %d of %d tail / partial-turn positions do not separate" % (n, int((~differ[at]).sum()), int(at.sum()))
        assert np.all(np.isfinite(e)) and np.all(np.isfinite(p))
        covered += int(at.sum())
    assert covered > turn
    # the positions: a vector arena of one turn + 7 floats has its last 4 + 3 outside the whole turn; an element-wise one its last 7
    assert list(np.flatnonzero(M.tail_and_partial_turn(turn + 7, turn, vector))) == list(range(turn, turn + 7))
    assert not M.tail_and_partial_turn(turn, turn, vector).any() and M.tail_and_partial_turn(turn - 1, turn, vector).all()


def test_alternatives_are_what_their_names_say():
    e, p = _inputs()
    e, p = e[:4096], p[:4096]
    for w in WEIGHTS[:3]:
        unfused = (e + (w * (p - e)).astype(np.float32)).astype(np.float32) if w < 0.5 else \
            (p - ((p - e) * (np.float32(1) - w)).astype(np.float32)).astype(np.float32)
        assert np.array_equal(_bits(M.unfused32(e, p, w)), _bits(unfused))
    half = np.float32(0.5)
    assert np.array_equal(_bits(M.other_branch32(e, p, half)), _bits(M.fma32(half, p - e, e)))
    assert np.array_equal(_bits(M.alternative32(e, p, half)), _bits(M.other_branch32(e, p, half)))
    assert np.array_equal(_bits(M.alternative32(e, p, np.float32(0.8))), _bits(M.unfused32(e, p, np.float32(0.8))))


def test_ema_run_counts_and_skips():
    rng = np.random.RandomState(3)
    start = [rng.randn(7).astype(np.float32)]
    steps = [[rng.randn(7).astype(np.float32)] for _ in range(5)]
    run = M.ema_run(steps, start, 0.9, every=2)
    assert [c for _, c in run] == [0, 1, 1, 2, 2]
    assert np.array_equal(run[0][0][0], start[0]) and np.array_equal(run[1][0][0], run[2][0][0])
    assert np.array_equal(run[1][0][0], M.lerp32(start[0], steps[1][0], M.weight(0.9, False, 0)))
    off = M.ema_run(steps, start, 0.9, every=0)
    assert all(c == 0 and np.array_equal(a[0], start[0]) for a, c in off)
    warm = M.ema_run(steps, start, 0.9999, every=1, warmup=True)
    assert np.array_equal(warm[0][0][0], M.lerp32(start[0], steps[0][0], np.float32(0.9)))


def test_exports_and_prototypes():
    from resnet_amd import binding as B
    lib = C.CDLL(B.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "resnet_mi.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name + " is not exported"
        assert name in B.PROTOTYPES, name + " is not in binding.PROTOTYPES"
        assert name + "(" in header, name + " is not declared in include/resnet_mi.h"
    L = B.load()
    geo = (C.c_size_t * 4)()
    L.mi_debug_ema_geometry(geo)  # host only
    assert geo[0] == 256 and geo[1] == 4 * geo[2] and geo[3] >= 1


def test_kernels_optim_keeps_the_mutants_old_texts_unique():
    """tests/mutants.py replaces these lines of kernels_optim.hip; each must occur exactly once in the file"""
    src = open(os.path.join(ROOT, "resnet_amd", "csrc", "kernels_optim.hip")).read()
    for old in ("opt_elem<KIND>(w, q, b, s, wdt, lr, mu, skip, bad);", "else wdt = 0.f;", "tr = trust_coef * wn / (gn + wd * wn);"):
        assert src.count(old) == 1, old
    assert "ema_update_kernel" in src and "exchange_kernel" in src
