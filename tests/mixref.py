"""numpy / math restatement of mixing (include/resnet_mi.h, "mixing"): the plan of mi_mix_plan (Python ints and floats, math.pow /
math.sqrt scalars), the float32 mix of mi_op_mix_batch (kernels_input.hip) and the float64 and float32 two-label heads of
mi_op_loss_head_mix (kernels_loss.hip).  The one-label pieces (soft-max, rank rule, inputs, bound) are lossref's."""
import math

import numpy as np

import lossref

M64 = 0xFFFFFFFFFFFFFFFF
_G = 0x9E3779B97F4A7C15
TRIES = 64


def splitmix64_at(seed, i):
    """element i of the counter stream `seed` (synth.splitmix64, augref.splitmix64_at) on Python ints, i taken modulo 2^64"""
    z = (seed + ((i + 1) & M64) * _G) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def unit(x):
    """U(x) = (x >> 11) 2^-53"""
    return float(x >> 11) * 2.0 ** -53


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def plan(seed, epoch, step, rank, world, mixup_alpha, cutmix_alpha, prob, switch_prob, dim):
    """dict(mode, lam (np.float32), y0, x0, y1, x1, fallback): fallback = no try of Johnk's method was taken (lam = 0.5 before the box)"""
    assert mixup_alpha > 0 or cutmix_alpha > 0
    out = dict(mode=0, lam=np.float32(1.0), y0=0, x0=0, y1=0, x1=0, fallback=False)
    s = splitmix64_at(seed & M64, epoch)
    k = splitmix64_at(s, step * world + rank)
    if unit(splitmix64_at(k, 0)) >= prob:
        return out
    if mixup_alpha > 0 and cutmix_alpha > 0:
        cut_mode = unit(splitmix64_at(k, 1)) < switch_prob
    else:
        cut_mode = cutmix_alpha > 0
    inv = 1.0 / (cutmix_alpha if cut_mode else mixup_alpha)
    lam, out["fallback"] = 0.5, True
    for t in range(TRIES):
        X = math.pow(unit(splitmix64_at(k, 2 + 2 * t)), inv)
        Y = math.pow(unit(splitmix64_at(k, 3 + 2 * t)), inv)
        if 0 < X + Y <= 1:
            lam, out["fallback"] = X / (X + Y), False
            break
    out["mode"] = 2 if cut_mode else 1
    if cut_mode:
        D = dim
        cut = int(D * math.sqrt(1.0 - lam))
        cy = ((splitmix64_at(k, 130) >> 32) * D) >> 32
        cx = ((splitmix64_at(k, 131) >> 32) * D) >> 32
        out["y0"], out["y1"] = _clamp(cy - cut // 2, 0, D), _clamp(cy + cut // 2, 0, D)
        out["x0"], out["x1"] = _clamp(cx - cut // 2, 0, D), _clamp(cx + cut // 2, 0, D)
        lam = 1.0 - ((out["y1"] - out["y0"]) * (out["x1"] - out["x0"])) / (D * D)
    out["lam"] = np.float32(lam)
    return out


def clamp_box(y0, x0, y1, x1, D):
    """the box as the kernel clamps it"""
    y0 = _clamp(y0, 0, D)
    y1 = _clamp(max(y1, y0), 0, D)
    x0 = _clamp(x0, 0, D)
    x1 = _clamp(max(x1, x0), 0, D)
    return y0, x0, y1, x1


def mix(images, p):
    """the batch (n, 3, D, D) float32 mixed under plan p (a dict as plan() or Trainer.last_mix() gives it): row i with row n - 1 - i, the
    middle row of an odd batch untouched.  mode 1: every product and sum a float32 operation of its own; mode 2: the box changes places"""
    x = np.array(images, np.float32, copy=True)
    n, D = x.shape[0], x.shape[2]
    if p["mode"] == 0:
        return x
    if p["mode"] == 1:
        lam = np.float32(p["lam"])
        mu = np.float32(1.0) - lam
        with np.errstate(invalid="ignore", over="ignore"):
            for i in range(n // 2):
                a, b = x[i].copy(), x[n - 1 - i].copy()
                x[i] = lam * a + mu * b
                x[n - 1 - i] = lam * b + mu * a
        return x
    y0, x0, y1, x1 = clamp_box(p["y0"], p["x0"], p["y1"], p["x1"], D)
    for i in range(n // 2):
        a = x[i, :, y0:y1, x0:x1].copy()
        x[i, :, y0:y1, x0:x1] = x[n - 1 - i, :, y0:y1, x0:x1]
        x[n - 1 - i, :, y0:y1, x0:x1] = a
    return x


def labels_b(labels):
    """the partners' labels: labels_b[i] = labels[n - 1 - i]"""
    return np.ascontiguousarray(np.asarray(labels)[::-1])


def targets_f32(L, a, b, lam, eps):
    """t (N, L) float32 as the kernel adds it up: t_j = ((j == a ? wa : 0) + (j == b ? wb : 0)) + u, wa = (1 - eps) lam, wb = (1 - eps)
    (1 - lam), u = eps / L, every operation in float32.  a outside [0, L): no a term; b outside [0, L), or wb == 0: no b term"""
    f = np.float32
    lam, eps = f(lam), f(eps)
    u = eps / f(L)
    wa, wb = (f(1) - eps) * lam, (f(1) - eps) * (f(1) - lam)
    N = len(a)
    t = np.empty((N, L), f)
    for r in range(N):
        w = np.zeros(L, f)
        w2 = np.zeros(L, f)
        if 0 <= a[r] < L:
            w[a[r]] = wa
        if wb > 0 and 0 <= b[r] < L:
            w2[b[r]] = wb
        t[r] = (w + w2) + u
    return t


def loss_head_mix(x, a, b, lam, eps=0.0):
    """(pred, dlogits, row_loss, row_rank) in float64 / int64; lam and eps as given (the float32 lam widened).  The rank is label a's"""
    x = np.asarray(x, np.float64)
    N, L = x.shape
    lam = float(lam)
    u = eps / L
    wa, wb = (1.0 - eps) * lam, (1.0 - eps) * (1.0 - lam)
    z = x - x.max(axis=1, keepdims=True)
    s = np.exp(z).sum(axis=1)
    pred = np.exp(z) / s[:, None]
    t = np.full((N, L), u)
    row_loss = np.empty(N)
    for r in range(N):
        ca, cb = int(a[r]), int(b[r])
        ok_a, ok_b = 0 <= ca < L, 0 <= cb < L
        if ok_a:
            t[r, ca] += wa
        if wb > 0 and ok_b:
            t[r, cb] += wb
        if ok_a and (ok_b or not wb > 0):
            row_loss[r] = np.log(s[r]) - wa * z[r, ca] - (wb * z[r, cb] if wb > 0 else 0.0) - u * z[r].sum()
        else:
            row_loss[r] = np.nan
    return pred, pred - t, row_loss, lossref.rank_of(pred, a)


def loss_head_mix_f32(x, a, b, lam, eps=0.0):
    """row_loss by the kernel's own steps in float32 (lossref.loss_head_f32 with the second label's term): lane-strided sums of 64 lanes,
    the exchange tree, rows of more than 1024 columns adding z in double"""
    f = np.float32
    x = np.asarray(x, f)
    N, L = x.shape
    lam, epsf = f(lam), f(eps)
    u = epsf / f(L)
    wa, wb = (f(1) - epsf) * lam, (f(1) - epsf) * (f(1) - lam)
    out = np.empty(N, f)

    def tree(v):
        v = v.copy()
        o = 32
        while o:
            v = v + v[np.arange(64) ^ o]
            o >>= 1
        return v[0]

    for r in range(N):
        ca, cb = int(a[r]), int(b[r])
        mx = x[r].max()
        z = x[r] - mx
        e = np.exp(z)
        s_l, z_l = np.zeros(64, f), np.zeros(64, f if L <= 1024 else np.float64)
        for j in range(L):
            s_l[j % 64] += e[j]
            z_l[j % 64] += z[j]
        s, sz = tree(s_l), f(tree(z_l))
        ok_b = 0 <= cb < L
        if 0 <= ca < L and (ok_b or not wb > 0):
            zb = z[cb] if wb > 0 else f(0)
            out[r] = np.log(s) - wa * z[ca] - wb * zb - u * sz
        else:
            out[r] = np.nan
    return out


LAMS = [0.0, 0.3, 1.0]  # the operator tests' weights; 0.3 is no float32: np.float32(0.3) is what both sides see
# At lam = 0.3 with eps 0 or 0.1 every way of forming wb gives the same float32 ((1 - eps) (1 - lam), (1 - eps) - wa, 1 - (eps + wa), ...):
# those cases cannot tell how the kernel rounds it.  At lam = 0.7, eps = 0.1 the product (1 - eps) (x) (1 - lam) and the difference
# (1 - eps) (-) wa are neighbouring floats (tests/test_mix_model.py)
WB_LAM, WB_EPS = 0.7, 0.1


def wb_as_difference(lam, eps):
    """what the kernel must NOT compute: wb = (1 - eps) (-) wa"""
    f = np.float32
    return (f(1) - f(eps)) - (f(1) - f(eps)) * f(lam)


def targets_reassociated_f32(L, a, b, lam, eps):
    """targets_f32 with the sum associated the other way, t_j = wa_j + (wb_j + u): differs from targets_f32 only in rows with a == b"""
    f = np.float32
    lam, eps = f(lam), f(eps)
    u = eps / f(L)
    wa, wb = (f(1) - eps) * lam, (f(1) - eps) * (f(1) - lam)
    t = np.empty((len(a), L), f)
    for r in range(len(a)):
        w, w2 = np.zeros(L, f), np.zeros(L, f)
        if 0 <= a[r] < L:
            w[a[r]] = wa
        if wb > 0 and 0 <= b[r] < L:
            w2[b[r]] = wb
        t[r] = w + (w2 + u)
    return t
