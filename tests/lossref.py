"""float64 numpy model of the device loss head (include/resnet_mi.h, "the loss head on the device"; kernels_loss.hip).

Per row of logits x[0..L) with label c, smoothing eps and u = eps / L:
  pred      p = exp(x - mx) / sum exp(x - mx), mx = max x
  dlogits   p - t, t_c = (1 - eps) + u, t_j = u otherwise (a batch SUM: no 1/N)
  row_loss  log(sum exp(x - mx)) - (1 - eps) (x_c - mx) - u sum_j (x_j - mx)   = -sum_j t_j log p_j
  row_rank  #{ j != c : p_j >= p_c }  (ties count against the label; a NaN p_c compares false: rank 0)
A label outside [0, L): dlogits = p - u, row_rank = L, row_loss = NaN.
"""
import numpy as np


def softmax(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def rank_of(pred, labels):
    """the rank rule on GIVEN probabilities (any float type: the comparisons are exact)"""
    pred = np.asarray(pred)
    N, L = pred.shape
    out = np.empty(N, np.int64)
    for r in range(N):
        c = int(labels[r])
        if not 0 <= c < L:
            out[r] = L
            continue
        ge = pred[r] >= pred[r, c]
        ge[c] = False
        out[r] = int(ge.sum())
    return out


def host_rule_wrong(pred, labels):
    """mi_host_loss's top-1 rule (resnet.cu:3363-3383): a row is wrong when any other class has p >= p_c"""
    pred = np.asarray(pred)
    out = np.zeros(pred.shape[0], bool)
    for r in range(pred.shape[0]):
        c = int(labels[r])
        for j in range(pred.shape[1]):
            if j != c and pred[r, j] >= pred[r, c]:
                out[r] = True
                break
    return out


def loss_head(x, labels, eps=0.0):
    """(pred, dlogits, row_loss, row_rank) in float64 / int64"""
    x = np.asarray(x, np.float64)
    N, L = x.shape
    u = eps / L
    z = x - x.max(axis=1, keepdims=True)
    s = np.exp(z).sum(axis=1)
    pred = np.exp(z) / s[:, None]
    t = np.full((N, L), u)
    row_loss = np.empty(N)
    for r in range(N):
        c = int(labels[r])
        if 0 <= c < L:
            t[r, c] = (1.0 - eps) + u
            row_loss[r] = np.log(s[r]) - (1.0 - eps) * z[r, c] - u * z[r].sum()
        else:
            row_loss[r] = np.nan
    return pred, pred - t, row_loss, rank_of(pred, labels)


SHAPES = [(2, 1), (3, 10), (5, 64), (4, 65), (8, 1000), (7, 1537)]  # (N, L): see tests/test_gpu_loss_head.py
TIE_ROW, UNDERFLOW_ROW = 1, 0


def make_inputs(N, L):
    """the logits and labels of the loss-head tests: N(0, 9) logits (seed 51) with the overflow hazard x[3, 17] = 95 where it exists,
    labels from seed 52; L >= 2: row 0's label logit 110 below the row's maximum (p_c = 0 in fp32); L >= 3: row 1 integer-valued with
    exactly two other classes at the label's logit and every other class below it (rank 2)"""
    import synth
    x = synth.normal(51, N * L, 9.0).reshape(N, L).copy()
    lab = synth.labels(52, N, L)
    if N > 3 and L > 17:
        x[3, 17] = 95.0
    if L >= 2:
        c = int(lab[UNDERFLOW_ROW])
        x[UNDERFLOW_ROW, c] = np.delete(x[UNDERFLOW_ROW], c).max() - np.float32(110.0)
    if L >= 3:
        c = int(lab[TIE_ROW])
        x[TIE_ROW] = (np.arange(L) % 4).astype(np.float32)
        x[TIE_ROW, [c, (c + 1) % L, (c + 2) % L]] = 4.0
    return np.ascontiguousarray(x, np.float32), lab


def dominant_inputs(L):
    """(x, labels) of test_gpu_loss_head.py::test_dominant_logit_past_column_63: ewref.dominant_rows / dominant_labels -- per row one
    logit 95 above every other at a column past 63 (the last row has none); labels on it, past column 63 off it, at column 0"""
    import ewref
    return ewref.dominant_rows(L), ewref.dominant_labels(L)


def loss_head_f32_max_of(x, labels, eps, cols):
    """loss_head_f32's row_loss with the row maximum taken over the first `cols` columns only (the planted faults of tests/mutants.py that
    leave a lane's later turns out of the maximum): float32 throughout, so a logit far above that maximum overflows exp"""
    f = np.float32
    x = np.asarray(x, f)
    N, L = x.shape
    u = f(eps) / f(L)
    out = np.empty(N, f)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(N):
            c = int(labels[r])
            z = x[r] - x[r, :cols].max()
            s = np.exp(z).sum(dtype=f)
            out[r] = np.log(s) - (f(1) - f(eps)) * z[c] - u * z.sum(dtype=f)
    return out


RANKED_SHAPE = (130, 10)  # 130 rows: the 64 lanes of loss_reduce_kernel take three passes, the last with rows 128 and 129 only


def ranked_inputs():
    """(x, labels, ranks) for the batch totals: row r of RANKED_SHAPE holds a permutation (seed 53) of the logits 0 .. L - 1 and its
    label is the class with the (r mod L)-th largest logit, so row_rank[r] == r mod L by construction -- every value of the rank
    occurs, in the rows below 64 and in the rows past them.  Distinct integers: no ties, nothing underflows (the smallest p is e^-9 / s)"""
    N, L = RANKED_SHAPE
    rng = np.random.RandomState(53)
    x = np.empty((N, L), np.float32)
    lab = np.empty(N, np.int32)
    for r in range(N):
        x[r] = rng.permutation(L)
        lab[r] = int(np.argsort(-x[r])[r % L])
    return x, lab, np.arange(N) % L


RANKED_COUNTS = {1: (117, 117), 5: (117, 65), 10: (117, 0)}  # topk -> (wrong_top1, wrong_topk) of ranked_inputs; rows past 64: 60 and 35


def check_batch_totals(head, new_total, topk):
    """the batch totals (loss_reduce_kernel) on ranked_inputs, for the one-label and the two-label operator alike: 130 rows -- three
    passes of the 64 lanes, the last with two rows -- whose ranks are arange(130) % 10 by construction, so that rows with rank == topk
    exist and the rows past 64 hold 60 and 35 of the counts.  head(x, labels, total) launches the operator with this topk and returns what
    Ops.loss_head returns; new_total() is a zeroed record on the device.  Asserts row_rank, the counts, loss_sum against the float64 sum
    of the device's own row_loss (1e-12 relative: a lane that adds its rows in float is 5e-9 off), and that a second launch doubles total"""
    x, lab, ranks = ranked_inputs()
    N = len(lab)
    total = new_total()
    pred, dl, rl, rr, last, tot = head(x, lab, total)
    assert np.array_equal(rr, ranks), "row_rank is not the constructed vector: rows %s" % np.flatnonzero(rr != ranks)[:8]
    w1, wk = RANKED_COUNTS[topk]
    assert (w1, wk) == (int(np.sum(ranks >= 1)), int(np.sum(ranks >= topk)))
    assert (last["rows"], last["wrong_top1"], last["wrong_topk"], last["batches"]) == (N, w1, wk, 1), last
    assert np.all(np.isfinite(rl))
    want = float(np.sum(rl.astype(np.float64)))
    assert abs(last["loss_sum"] - want) <= 1e-12 * abs(want), (last["loss_sum"], want)
    assert tot == last
    again = head(x, lab, total)
    assert again[4] == last and np.float64(again[4]["loss_sum"]).tobytes() == np.float64(last["loss_sum"]).tobytes()
    assert again[5]["loss_sum"] == 2 * last["loss_sum"] and again[5]["batches"] == 2
    assert all(again[5][f] == 2 * last[f] for f in ("rows", "wrong_top1", "wrong_topk")), again[5]
    return pred, dl, rl


def loss_bound(ref):
    """|device row_loss - ref| allowed per row: 2^-19 (2 + ref) (derivation: DESIGN.md, "Loss head")"""
    return 2.0 ** -19 * (2.0 + np.asarray(ref, np.float64))


def loss_bound_mem(x, labels, eps):
    """the first-order bound DESIGN.md ("Loss head") derives for loss_head_kernel<mem> (L > 1024, lanes add z in double), per row, before
    it is rounded up to loss_bound's 64 + 32 ref:  2^-24 (ln L + 2 + (m + 5) + 4 ls + 5 a + 6 b),  m = ceil(L / 64), ls = log s,
    a = (1 - eps) |z_c|, b = eps mean |z_j|"""
    x = np.asarray(x, np.float64)
    N, L = x.shape
    z = x - x.max(axis=1, keepdims=True)
    ls = np.log(np.exp(z).sum(axis=1))
    a = (1.0 - eps) * np.abs(z[np.arange(N), labels])
    b = eps * np.abs(z).mean(axis=1)
    return 2.0 ** -24 * (np.log(L) + 2.0 + (-(-L // 64) + 5) + 4.0 * ls + 5.0 * a + 6.0 * b)


LONG_ROW_L = 1537
LONG_ROW_T = (90.0, 120.0, 150.0, 180.0, 240.0)


def long_row_corner():
    """(x, labels): the corner the double lane sums of loss_head_kernel<mem> close ("Loss head": label at the maximum, every other
    logit far below it, smoothing 0.5, so that u sum z is nearly all of the loss), one row of LONG_ROW_L columns per T in LONG_ROW_T.  The label is
    the last column, logit 0; lane l of the kernel adds columns l, l + 64, ...: column j holds -t[j // 64] with t[0] = T and t[k] the
    float among the 64 next above T whose addition to the running FLOAT sum t[0] + ... + t[k-1] loses the most (almost half an ulp of the
    sum, every time downwards).  A float lane sum is then off by about 9 x 2^-24 relative, where the double sum is exact"""
    f = np.float32
    rows = []
    for T in LONG_ROW_T:
        t, p = [f(T)], f(T)
        for _ in range(1, LONG_ROW_L // 64):
            cands = f(T) + np.arange(64, dtype=f) * np.spacing(f(T))
            lost = (np.float64(p) + cands.astype(np.float64)) - (p + cands).astype(np.float64)
            c = cands[int(np.argmax(lost))]
            t.append(c)
            p = f(p + c)
        x = -np.asarray(t, f)[np.minimum(np.arange(LONG_ROW_L) // 64, len(t) - 1)]
        x[-1] = 0.0
        rows.append(x)
    return np.ascontiguousarray(rows, f), np.full(len(rows), LONG_ROW_L - 1, np.int32)


def loss_head_f32(x, labels, eps=0.0, long_rows_in_double=True):
    """the kernel's own formulas step by step in float32 (lane-strided sums of 64 lanes, then the exchange tree): row_loss only.  Used to hold
    the derived bound against fp32 arithmetic without a GPU.  long_rows_in_double = False: the lanes of a row of more than 1024 columns add
    z in float (what the kernel must NOT do: tests/test_loss_model.py shows the bound of the long-row corner then fails)"""
    f = np.float32
    x = np.asarray(x, f)
    N, L = x.shape
    epsf = f(eps)
    u = epsf / f(L)
    out = np.empty(N, f)

    def tree(v):
        v = v.copy()
        o = 32
        while o:
            v = v + v[np.arange(64) ^ o]
            o >>= 1
        return v[0]

    for r in range(N):
        c = int(labels[r])
        mx = x[r].max()
        z = x[r] - mx
        e = np.exp(z)  # numpy's float32 exp: within 1 ulp, as expf
        s_l, z_l = np.zeros(64, f), np.zeros(64, f if L <= 1024 or not long_rows_in_double else np.float64)  # a row of more than 16 per lane sums z in double
        for j in range(L):
            s_l[j % 64] += e[j]
            z_l[j % 64] += z[j]
        s, sz = tree(s_l), f(tree(z_l.astype(np.float64) if L > 1024 else z_l))
        out[r] = np.log(s) - (f(1) - epsf) * z[c] - u * sz if 0 <= c < L else np.nan
    return out
