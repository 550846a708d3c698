"""The float64 model of the device loss head (tests/lossref.py) against torch's label-smoothed cross entropy and its autograd gradient, the
model's rank rule against mi_host_loss's top-1 rule, the derived row-loss bound against an fp32 restatement of the kernel's formulas, and
the library's exports.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lossref as R


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_model_equals_torch_cross_entropy_and_its_gradient(shape, eps):
    x, lab = R.make_inputs(*shape)
    pred, dlogits, row_loss, _ = R.loss_head(x, lab, eps)
    t = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tl = torch.tensor(lab, dtype=torch.long)
    rows = F.cross_entropy(t, tl, label_smoothing=eps, reduction="none")
    assert np.max(np.abs(row_loss - rows.detach().numpy()) / (1.0 + rows.detach().numpy())) <= 1e-12
    F.cross_entropy(t, tl, label_smoothing=eps, reduction="sum").backward()
    assert np.max(np.abs(dlogits - t.grad.numpy())) <= 1e-12
    assert np.max(np.abs(pred - torch.softmax(t.detach(), dim=1).numpy())) <= 1e-14
    assert np.all(np.isfinite(row_loss))


@pytest.mark.parametrize("shape", R.SHAPES)
def test_rank_rule(shape):
    N, L = shape
    x, lab = R.make_inputs(N, L)
    pred, _, _, rank = R.loss_head(x, lab)
    assert np.array_equal(rank >= 1, R.host_rule_wrong(pred, lab))
    if L >= 3:
        assert rank[R.TIE_ROW] == 2
    if L == 1:
        assert not rank.any()
    p32 = pred.astype(np.float32)
    if L >= 2:
        assert p32[R.UNDERFLOW_ROW, lab[R.UNDERFLOW_ROW]] == 0  # every other class ties with or beats a zero
        assert R.rank_of(p32, lab)[R.UNDERFLOW_ROW] == L - 1
    nan = p32.copy()
    nan[0, lab[0]] = np.nan  # a NaN p_c compares false with everything, in both rules
    assert R.rank_of(nan, lab)[0] == 0 and not R.host_rule_wrong(nan, lab)[0]


def test_ranked_inputs_have_the_ranks_they_are_built_for():
    """lossref.ranked_inputs (the batch-totals test): with the float32 soft-max the ranks are arange(N) % L; the counts the operator test
    asserts follow, and the rows past the 64 lanes carry a share of each, so that a reduction that loses them shows.  None of
    lossref.SHAPES has a row whose rank equals its top-k: `rank >= k` written `> k` gives the same counts there"""
    x, lab, ranks = R.ranked_inputs()
    N, L = R.RANKED_SHAPE
    assert x.shape == (N, L) and N > 128 and np.array_equal(ranks, np.arange(N) % L)
    assert all(sorted(row) == list(range(L)) for row in x)
    e = np.exp(x - x.max(axis=1, keepdims=True))  # float32 throughout
    p32 = e / e.sum(axis=1, keepdims=True)
    assert p32.dtype == np.float32 and np.array_equal(R.rank_of(p32, lab), ranks)
    assert np.array_equal(R.loss_head(x, lab)[3], ranks)
    assert [int(np.sum(ranks >= k)) for k in (1, 5, 10)] == [117, 65, 0]
    assert [int(np.sum(ranks[64:] >= k)) for k in (1, 5)] == [60, 35]
    for k in (1, 5):
        assert int(np.sum(ranks > k)) != int(np.sum(ranks >= k))
    for shape in R.SHAPES:
        xs, ls = R.make_inputs(*shape)
        pr = R.softmax(xs).astype(np.float32)
        assert not np.any(R.rank_of(pr, ls) == min(5, shape[1])), shape
    # a lane that adds its two or three rows in float is off by far more than the 1e-12 the operator test allows
    for eps in (0.0, 0.1):
        rl = R.loss_head_f32(x, lab, eps)
        lanes = np.zeros(64, np.float32)
        for r in range(N):
            lanes[r % 64] += rl[r]
        want = float(np.sum(rl.astype(np.float64)))
        assert abs(float(np.sum(lanes.astype(np.float64))) - want) > 1e-10 * want


def test_labels_outside_the_row():
    x, lab = R.make_inputs(3, 10)
    bad = lab.copy()
    bad[0], bad[2] = -1, 10
    pred, dlogits, row_loss, rank = R.loss_head(x, bad, 0.1)
    good = R.loss_head(x, lab, 0.1)
    assert np.array_equal(pred, good[0]) and np.array_equal(dlogits[1], good[1][1]) and row_loss[1] == good[2][1]
    assert rank[0] == 10 and rank[2] == 10 and np.isnan(row_loss[0]) and np.isnan(row_loss[2])
    assert np.array_equal(dlogits[[0, 2]], pred[[0, 2]] - 0.1 / 10)


@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_fp32_formulas_stay_inside_the_derived_bound(shape, eps):
    x, lab = R.make_inputs(*shape)
    ref = R.loss_head(x, lab, eps)[2]
    got = R.loss_head_f32(x, lab, eps).astype(np.float64)
    share = np.max(np.abs(got - ref) / R.loss_bound(ref))
    print("fp32 formulas, %s eps %g: worst |error| / bound = %.4f" % (shape, eps, share))
    assert np.all(np.isfinite(got)) and share <= 0.06  # the share the bound's derivation leaves unused: DESIGN.md


def test_long_row_corner_needs_the_double_lane_sums():
    """the rows of lossref.long_row_corner against the first-order <mem> bound of DESIGN.md (lossref.loss_bound_mem, tighter than loss_bound):
    the fp32 restatement with double lane sums stays inside it with room, the same formulas with float lane sums do not -- the check
    tests/test_gpu_loss_head.py::test_long_row_sums_z_in_double makes on the device"""
    x, lab = R.long_row_corner()
    assert x.shape == (len(R.LONG_ROW_T), R.LONG_ROW_L) and x.shape[1] > 1024
    eps = 0.5
    ref = R.loss_head(x, lab, eps)[2]
    bound = R.loss_bound_mem(x, lab, eps)
    assert np.all(bound < R.loss_bound(ref))
    good = np.abs(R.loss_head_f32(x, lab, eps).astype(np.float64) - ref) / bound
    bad = np.abs(R.loss_head_f32(x, lab, eps, long_rows_in_double=False).astype(np.float64) - ref) / bound
    print("double lane sums: worst |error| / bound %.3f; float lane sums: %s" % (good.max(), np.round(bad, 3)))
    assert good.max() <= 0.5
    assert np.all(bad > 1.0)


def test_library_exports_the_loss_entry_points():
    from resnet_amd import binding
    lib = binding.load()
    for name in ("mi_op_loss_head", "mi_trainer_set_loss", "mi_trainer_metrics"):
        assert hasattr(lib, name) and name in binding.PROTOTYPES, name
    import ctypes as C
    assert C.sizeof(binding.MiLossMetrics) == 40
