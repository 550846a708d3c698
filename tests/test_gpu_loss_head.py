"""The loss head on the device (include/resnet_mi.h, "the loss head on the device"; kernels_loss.hip) through mi_op_loss_head, against
mi_op_softmax / mi_op_ce_deriv bit for bit and the float64 model of lossref.py.

Shapes (N, L), the smallest at which the kernel can go wrong: (2, 1) s = 1, loss 0, rank 0; (3, 10) fewer than 64 columns, idle lanes;
(5, 64), (4, 65) the lane-stride boundary; (8, 1000) the workload's row; (7, 1537) a row longer than the 16 elements per lane the kernel
keeps in registers.  Inputs (lossref.make_inputs): N(0, 9) logits with x[3, 17] = 95 (the overflow hazard of test_softmax_ce_adam), a row
whose label logit is 110 below the maximum (p_c = 0 in fp32), an integer-valued row in which two other classes tie with the label.

row_loss against the float64 model: |got - ref| <= 2^-19 (2 + ref) per row, derived in DESIGN.md ("Loss head") from the roundings of the
kernel's formulas, not measured; tests/test_loss_model.py holds an fp32 restatement of the formulas under 0.06 of it.
"""
import ctypes as C

import numpy as np
import pytest

import convref
import ewref
import lossref as R
from util import ACT_MAX_ABS, ACT_REL_L2, check_act

pytestmark = pytest.mark.gpu

EPS = [0.0, 0.1, 0.5]
_SOFTMAX = {}  # shape -> (x, labels, ops.softmax(x)): computed once, never written


def _case(ops, shape):
    if shape not in _SOFTMAX:
        x, lab = R.make_inputs(*shape)
        _SOFTMAX[shape] = (x, lab, ops.softmax(x))
    return _SOFTMAX[shape]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _record():
    from resnet_amd import binding as B
    return np.zeros(C.sizeof(B.MiLossMetrics), np.uint8)  # a zeroed MiLossMetrics


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_loss_head(ops, shape, eps):
    N, L = shape
    x, lab, sm = _case(ops, shape)
    k = min(5, L)
    total = ops.dev(_record())
    pred, dl, rl, rr, last, tot1 = ops.loss_head(x, lab, eps, k, total=total)
    # pred: the bits of the soft-max operator; dlogits: the bits of ce_deriv (eps 0), the model (eps > 0)
    assert _same(pred, sm), "pred differs from mi_op_softmax in %d elements" % int(np.sum(_bits(pred) != _bits(sm)))
    ref_pred, ref_dl, ref_loss, _ = R.loss_head(x, lab, eps)
    if eps == 0.0:
        assert _same(dl, ops.ce_deriv(sm, lab))
    else:
        check_act(dl, ref_dl, "dlogits %s eps %g" % (shape, eps), ACT_REL_L2, ACT_MAX_ABS)
    # rank: the model's rule on the device's own pred
    assert np.array_equal(rr, R.rank_of(pred, lab))
    if L >= 3:
        assert rr[R.TIE_ROW] == 2
    alive = pred[np.arange(N), lab] > 0
    if L >= 2:
        assert not alive[R.UNDERFLOW_ROW]
    assert np.array_equal((rr >= 1)[alive], R.host_rule_wrong(pred, lab)[alive])
    # row loss: finite everywhere, inside the derived bound
    err = np.abs(rl.astype(np.float64) - ref_loss)
    print("row_loss %s eps %g: worst |error| / bound = %.4f" % (shape, eps, float(np.max(err / R.loss_bound(ref_loss)))))
    assert np.all(np.isfinite(rl))
    assert np.all(err <= R.loss_bound(ref_loss)), (err, R.loss_bound(ref_loss))
    # the records
    want = float(np.sum(rl.astype(np.float64)))
    assert abs(last["loss_sum"] - want) <= 1e-12 * abs(want)
    assert (last["rows"], last["wrong_top1"], last["wrong_topk"], last["batches"]) == (N, int(np.sum(rr >= 1)), int(np.sum(rr >= k)), 1)
    assert tot1 == last
    # the same launch again into the same total: identical bits everywhere, total = twice last
    pred2, dl2, rl2, rr2, last2, tot2 = ops.loss_head(x, lab, eps, k, total=total)
    assert _same(pred2, pred) and _same(dl2, dl) and _same(rl2, rl) and np.array_equal(rr2, rr) and last2 == last
    assert np.float64(last2["loss_sum"]).tobytes() == np.float64(last["loss_sum"]).tobytes()
    assert tot2["loss_sum"] == 2 * last["loss_sum"] and tot2["batches"] == 2
    assert all(tot2[f] == 2 * last[f] for f in ("rows", "wrong_top1", "wrong_topk"))
    # k = 1: top-k is top-1
    last1 = ops.loss_head(x, lab, eps, 1)[4]
    assert last1["wrong_topk"] == last1["wrong_top1"] == last["wrong_top1"] and last1["loss_sum"] == last["loss_sum"]


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("topk", [1, 5, 10])
def test_batch_totals_past_64_rows_and_at_the_topk_threshold(ops, topk, eps):
    """loss_reduce_kernel: lossref.check_batch_totals says what is built and asserted"""
    pred, dl, rl = R.check_batch_totals(lambda x, lab, total: ops.loss_head(x, lab, eps, topk, total=total), lambda: ops.dev(_record()), topk)
    x, lab, _ = R.ranked_inputs()
    assert _same(pred, ops.softmax(x))
    ref = R.loss_head(x, lab, eps)[2]
    assert np.all(np.abs(rl.astype(np.float64) - ref) <= R.loss_bound(ref))


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("L", ewref.DOMINANT_L)
def test_dominant_logit_past_column_63(ops, L, eps):
    """the row maximum is taken over j = lane, lane + 64, ...: make_inputs' large logit sits at column 17, in every lane's first turn, and
    a maximum that stops after it is the same function up to rounding.  lossref.dominant_inputs: rows whose only large logit -- 95 above
    every other one, so that expf overflows without it -- sits at column 64, at the last column, in between and (L > 960) in the last
    register slot of loss_head_kernel<reg>, with labels on it, past column 63 off it, and at column 0.  L = 65 and 1000 run <reg>, 1537
    <mem>.  Checks as test_loss_head: pred is the soft-max operator's bits and within the soft-max bound of float64, the rank is the rule
    on pred, row_loss inside loss_bound"""
    x, lab = R.dominant_inputs(L)
    pred, dl, rl, rr, last, _ = ops.loss_head(x, lab, eps, min(5, L))
    assert _same(pred, ops.softmax(x))
    ref_sm, A = ewref.softmax_ref(x)
    w, bad = convref.dist_f32(pred, ref_sm, A)
    assert bad == 0, "pred: %d out of the soft-max bound (worst %.3g)" % (bad, w)
    assert np.array_equal(rr, R.rank_of(pred, lab))
    assert rr[0] == 0 and rr[1] >= 1, "row 0's label is its dominant column, row 1's is not"
    ref_pred, ref_dl, ref_loss, _ = R.loss_head(x, lab, eps)
    check_act(dl, ref_dl, "dlogits L %d eps %g" % (L, eps), ACT_REL_L2, ACT_MAX_ABS)
    err = np.abs(rl.astype(np.float64) - ref_loss)
    assert np.all(np.isfinite(rl))
    assert np.all(err <= R.loss_bound(ref_loss)), (err, R.loss_bound(ref_loss))


def test_long_row_sums_z_in_double(ops):
    """loss_head_kernel<mem> (rows of more than 1024 columns) adds z per lane in double.  lossref.long_row_corner builds the corner that
    needs it: label at the maximum, every other logit 90 .. 240 below it, smoothing 0.5 (u sum z is nearly all of the loss), the logits
    chosen so that a FLOAT lane sum loses almost half an ulp at every addition.  Bound: the first-order <mem> bound DESIGN.md derives
    (lossref.loss_bound_mem: 2^-24 (ln L + 2 + m + 5 + 4 ls + 5 a + 6 b), about a fifth of loss_bound here), not loss_bound's rounded-up
    64 + 32 ref, which float lane sums also meet.  tests/test_loss_model.py: the fp32 restatement with double lanes uses 0.18 of it, with
    float lanes 1.3 to 1.4 times it"""
    x, lab = R.long_row_corner()
    eps = 0.5
    pred, dl, rl, rr, last, _ = ops.loss_head(x, lab, eps, 5)
    assert _same(pred, ops.softmax(x))
    assert not rr.any(), "the label is every row's only maximum"
    ref = R.loss_head(x, lab, eps)[2]
    share = np.abs(rl.astype(np.float64) - ref) / R.loss_bound_mem(x, lab, eps)
    print("row_loss of the long-row corner: |error| / <mem> bound = %s" % np.round(share, 3))
    assert np.all(np.isfinite(rl))
    assert np.all(share <= 1.0), "row_loss out of bounds: |error| / bound %s" % np.round(share, 3)


def _bad_labels(lab, L):
    bad = lab.copy()
    bad[0], bad[-1] = -1, L
    return bad


def _check_bad_labels(ops, shape, eps, good):
    N, L = shape
    x, lab, _ = _case(ops, shape)
    pred, dl, rl, rr, last, _ = ops.loss_head(x, _bad_labels(lab, L), eps, min(5, L))
    u = np.float32(eps) / np.float32(L)
    mid = slice(1, N - 1)
    assert _same(pred, good[0])
    assert rr[0] == L and rr[-1] == L and np.isnan(rl[0]) and np.isnan(rl[-1])
    assert _same(dl[[0, -1]], pred[[0, -1]] - u)
    assert _same(dl[mid], good[1][mid]) and _same(rl[mid], good[2][mid]) and np.array_equal(rr[mid], good[3][mid])
    assert last["rows"] == N and last["wrong_top1"] == int(np.sum(rr >= 1)) and np.isnan(last["loss_sum"])


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("shape", R.SHAPES)
def test_labels_outside_the_row(ops, shape, eps):
    x, lab, _ = _case(ops, shape)
    _check_bad_labels(ops, shape, eps, ops.loss_head(x, lab, eps, min(5, shape[1])))


@pytest.mark.parametrize("shape", [(3, 10), (4, 65)])
def test_stays_inside_its_tensors(ops, shape):
    """every tensor of the launch between two 4096-byte zones of 0xFF (NaN as fp32, -1 as a label), bad labels included, the way
    tests/test_gpu_redzone.py runs the other operators"""
    x, lab, _ = _case(ops, shape)
    plain = ops.loss_head(x, lab, 0.1, min(5, shape[1]))
    assert ops.L.mi_debug_redzone(4096, 0xFF) == 0
    try:
        zoned = ops.loss_head(x, lab, 0.1, min(5, shape[1]))
        _check_bad_labels(ops, shape, 0.1, plain)
        assert ops.L.mi_debug_redzone_check() == 0, ops.L.mi_last_error().decode()
    finally:
        assert ops.L.mi_debug_redzone(0, 0) == 0
    assert all(_same(a, b) for a, b in zip(zoned[:4], plain[:4])) and zoned[4] == plain[4]


def test_reads_no_stale_lds(ops):
    """with 0xFFFFFFFF in every LDS word behind every launch, every output keeps its bits"""
    shape = (8, 1000)
    x, lab, _ = _case(ops, shape)
    plain = ops.loss_head(x, lab, 0.1, 5)
    assert ops.L.mi_debug_lds_fill_mode(1, 0xFFFFFFFF) == 0, ops.L.mi_last_error()
    try:
        filled = ops.loss_head(x, lab, 0.1, 5)
        assert ops.L.mi_debug_lds_fills() >= 2  # behind the head and behind the reduce
    finally:
        assert ops.L.mi_debug_lds_fill_mode(0, 0) == 0
    assert all(_same(a, b) for a, b in zip(filled[:4], plain[:4])) and filled[4] == plain[4] and filled[5] == plain[5]


def test_null_outputs(ops):
    """every output may be NULL: the others keep their bits, and the records come out without the row outputs"""
    from resnet_amd import binding as B
    shape = (4, 65)
    N, L = shape
    x, lab, _ = _case(ops, shape)
    full = ops.loss_head(x, lab, 0.1, 5)
    dx, dlab = ops.dev(x), ops.dev(lab)
    outs = [ops.dev(shape=shape), ops.dev(shape=shape), ops.dev(shape=(N,)), ops.dev(shape=(N,), dtype=np.int32), ops.dev(_record()), ops.dev(_record())]
    for keep in range(6):
        ptrs = [o.ptr if i == keep else None for i, o in enumerate(outs)]
        ops._chk(ops.L.mi_op_loss_head(dx.ptr, dlab.ptr, *ptrs[:4], N, L, 0.1, 5, *ptrs[4:]), "loss_head")
        got = outs[keep].get()
        if keep < 4:
            assert _same(got, full[keep]), keep
        else:
            assert B.MiLossMetrics.from_buffer_copy(got.tobytes()).as_dict() == full[4], keep  # (a zeroed total: total == last)
    ops._chk(ops.L.mi_op_loss_head(dx.ptr, dlab.ptr, None, None, None, None, N, L, 0.1, 5, None, None), "loss_head")


@pytest.mark.parametrize("eps,k,n,l,word", [(1.0, 5, 4, 65, "smoothing"), (-0.1, 5, 4, 65, "smoothing"), (float("nan"), 5, 4, 65, "smoothing"),
                                            (0.1, 0, 4, 65, "topk"), (0.1, 66, 4, 65, "topk"), (0.1, 1, 0, 65, "N and L"), (0.1, 1, 4, 0, "N and L")])
def test_bad_arguments(ops, eps, k, n, l, word):
    x, lab, _ = _case(ops, (4, 65))
    dx, dlab, dp = ops.dev(x), ops.dev(lab), ops.dev(shape=x.shape)
    before = dp.get()
    assert ops.L.mi_op_loss_head(dx.ptr, dlab.ptr, dp.ptr, None, None, None, n, l, eps, k, None, None) == -1
    msg = ops.L.mi_last_error().decode()
    ops.L.mi_clear_error()
    assert "mi_op_loss_head" in msg and word in msg, msg
    assert _same(dp.get(), before)  # nothing was launched
