"""tests/accumref.py against torch on the CPU: a window of k micro-batch gradients is k - 1 in-place float32 additions onto a copy of the
first and one multiplication by the scale.  No GPU.  Bit for bit; a NaN matches any NaN (accumref.same says why), and the copy that
starts a window keeps even those bits."""
import numpy as np
import pytest
import torch

import accumref as M

SCALES = [np.float32(1.0), np.float32(0.25), np.float32(1.0) / np.float32(3.0)]
DENORMAL = np.float32(1e-40)
TINY = np.finfo(np.float32).tiny
HUGE = np.finfo(np.float32).max


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gradients(k, n=257, seed=0):
    """k arrays of n float32: random values of mixed magnitude, and at fixed places +-0, denormals, +-inf, NaN (a payload among them), pairs
    that cancel exactly, pairs whose sum overflows and sums that end below the normal range"""
    rng = np.random.RandomState(seed + 10 * k)
    gs = [(rng.randn(n) * 10.0 ** rng.randint(-6, 6, size=n)).astype(np.float32) for _ in range(k)]
    special = [0.0, -0.0, DENORMAL, -DENORMAL, np.inf, -np.inf, np.nan, TINY, -TINY, HUGE, -HUGE, 1.0, 3.0]
    for j, g in enumerate(gs):
        for i, v in enumerate(special):
            g[i] = v
            g[40 + i] = special[(i + j) % len(special)]  # every special value meets every other across the micro-batches
        g[80] = np.float32(1.5) if j % 2 == 0 else np.float32(-1.5)  # cancels for even k
        g[81] = HUGE if j < 2 else np.float32(0.0)                    # overflows for k >= 2
        g[82] = TINY if j == 0 else (-TINY / 2 if j == 1 else np.float32(0.0))  # a denormal sum
        g[83] = -0.0
    gs[0].view(np.uint32)[84] = 0x7FC12345  # a NaN payload and a signalling NaN in the first: the copy keeps them
    gs[0].view(np.uint32)[85] = 0xFF800001
    return gs


def _torch_window(gs, scale):
    acc = torch.from_numpy(gs[0].copy())
    for g in gs[1:]:
        acc.add_(torch.from_numpy(g))
    acc.mul_(float(scale))  # a Python scalar: the tensor stays float32 and the product is one float32 operation
    return acc.numpy()


def test_torch_keeps_denormals_here():
    a = torch.from_numpy(np.array([TINY], np.float32))
    assert float(a.mul_(0.5)) == float(TINY / 2) != 0.0, "the CPU flushes denormals: the pin below would be against another arithmetic"


@pytest.mark.parametrize("scale", SCALES, ids=["scale=%g" % s for s in SCALES])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_window_is_torch_add_then_mul(k, scale):
    gs = _gradients(k)
    assert float(np.float32(float(scale))) == float(scale)
    got, want = M.window(gs, scale), _torch_window(gs, scale)
    assert got.dtype == np.float32 and M.same(got, want), "%d elements differ" % int(np.sum(_bits(got) != _bits(want)))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    finite = np.isfinite(want)
    assert finite.sum() > 200 and np.array_equal(_bits(got)[finite], _bits(want)[finite])


def test_the_modes_one_by_one():
    g0, g1, g2 = _gradients(3, seed=4)
    acc = M.first(g0)
    assert np.array_equal(_bits(acc), _bits(g0)) and acc is not g0, "first: the words of g"
    assert _bits(acc)[84] == 0x7FC12345 and _bits(acc)[85] == 0xFF800001 and _bits(acc)[1] == 0x80000000
    acc2 = M.add(acc, g1)
    assert M.same(acc2, torch.from_numpy(g0.copy()).add_(torch.from_numpy(g1)).numpy())
    assert np.array_equal(_bits(acc), _bits(g0)), "add returns a new array"
    assert M.same(M.accumulator([g0, g1]), acc2)
    for scale in SCALES:
        f = M.fold(acc2, g2, scale)
        assert M.same(f, _torch_window([g0, g1, g2], scale)) and M.same(f, M.window([g0, g1, g2], scale))
    # uint32 words are taken as the floats they encode
    assert np.array_equal(_bits(M.first(_bits(g0))), _bits(g0)) and M.same(M.add(_bits(g0), _bits(g1)), acc2)


def test_the_fold_is_a_sum_then_a_product_not_a_fused_multiply_add():
    """(a + b) * s with the sum rounded to float32 before the product is: the same expression rounded once at the end gives the float32
    next to it for some operands, and the model (and torch) are on the two-rounding side there"""
    rng = np.random.RandomState(7)
    a = rng.randn(4096).astype(np.float32)
    b = (rng.randn(4096) * 1e-4).astype(np.float32)
    s = SCALES[2]
    two = M.fold(a, b, s)
    once = ((a.astype(np.float64) + b.astype(np.float64)) * np.float64(s)).astype(np.float32)  # one rounding at the end
    assert np.any(_bits(two) != _bits(once)), "the operands do not tell the two apart"
    assert M.same(two, _torch_window([a, b], s))


@pytest.mark.parametrize("vector", [True, False], ids=["vector", "element-wise"])
def test_separating_inputs_separate_every_tail_and_partial_turn_position(vector):
    """a condition, not a measurement: at every length of tests/test_gpu_accum.py, every position of the n % 4 tail and of the partial turn
    (and every other one) tells the two-rounding fold from the fold rounded once, at the operator test's scale 1 / 3; acc != g everywhere,
    so a launch that reads one operand twice shows in ADD as well"""
    import ctypes as C
    import emaref
    from resnet_amd import binding as B
    geo = (C.c_size_t * 4)()
    B.load().mi_debug_accum_geometry(geo)  # host only
    turn = int(geo[1] if vector else geo[2])
    scale = SCALES[2]
    for n in sorted({1, 3, 4, 5, 1023, 1024, 1025, turn - 1, turn, turn + 1}):
        acc, g = M.separating_pair(n, scale, n)
        assert acc.size == g.size == n and acc.dtype == g.dtype == np.float32
        differ = _bits(M.fold(acc, g, scale)) != _bits(M.fold_once(acc, g, scale))
        at = emaref.tail_and_partial_turn(n, turn, vector)
        assert differ[at].all() and differ.all(), "n = %d: %d positions do not separate" % (n, int((~differ).sum()))
        assert np.all(acc != g) and np.all(_bits(M.add(acc, g)) != _bits(M.add(g, g)))
    # fold_once is the expression of the test above
    rng = np.random.RandomState(7)
    a, b = rng.randn(4096).astype(np.float32), (rng.randn(4096) * 1e-4).astype(np.float32)
    once = ((a.astype(np.float64) + b.astype(np.float64)) * np.float64(scale)).astype(np.float32)
    assert np.array_equal(_bits(M.fold_once(a, b, scale)), _bits(once))


def test_special_values_follow_ieee():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    a = np.array([inf, inf, -0.0, 0.0, DENORMAL, HUGE, 1.5, nan], np.float32)
    b = np.array([-inf, 1.0, -0.0, -0.0, DENORMAL, HUGE, -1.5, 1.0], np.float32)
    s = M.add(a, b)
    assert np.isnan(s[0]) and s[1] == inf and _bits(s)[2] == 0x80000000 and _bits(s)[3] == 0 and s[4] == np.float32(2) * DENORMAL != 0  # exact
    assert s[5] == inf and _bits(s)[6] == 0 and np.isnan(s[7])
    f = M.fold(a, b, np.float32(0.25))
    assert np.isnan(f[0]) and f[1] == inf and _bits(f)[2] == 0x80000000 and f[4] == (np.float32(2) * DENORMAL) * np.float32(0.25) != 0 and f[5] == inf
    assert not M.same(np.array([0.0], np.float32), np.array([-0.0], np.float32)) and M.same(np.array([nan]), _bits(np.array([0xFFC00001], np.uint32)))
