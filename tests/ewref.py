"""Float64 references and per-element bounds for the element-wise half of the training step (CPU only): batch norm forward and
backward, max-pool, average pool, soft-max, Adam.  The checks are convref's (dist_f32 / dist_bf16 / check_slabs: |got - ref| <=
C_FACTOR 2^-24 A, bf16 outputs between RNE(ref -/+ that bound)); what this module adds is each operation's reference and its A.

Batch norm (kernels_bn.hip), per channel c over M = N * P samples, statistics (mean, biased var) given or produced:
  * statistics: mean and var in float64 over every sample of the slab's channels; A = mean |x|, mean x^2 (sum of |terms| / M)
  * apply: ref = g (x - mean) / sqrt(var + eps) + b (+ r), ReLU; A = APPLY_TERMS |g x_hat| + |b| (+ |r|) -- the kernel's own statistics
    are the contract (backward reuses them), so the reference takes the statistics the kernel was given or produced
  * dbeta = sum g_i, dgamma = sum g_i x_hat_i with g_i the gated gradient; A = sum of |terms| (convref.bn_grad_sums)
  * dx = (gamma / sd) (g_i - k1 - x_hat k2), k1 = dbeta / M, k2 = dgamma / M from the float64 sums;
    A = |gamma / sd| (DX_TERMS (|g_i| + |k1| + |x_hat k2|) + (sum |g|) / M + |x_hat| (sum |g x_hat|) / M): the second half is what the
    bounds of the two sums carry into dx
Max-pool (3x3, stride 2, pad 1, kernels_misc.hip) is restated exactly: strict '>' from -1024 in (r, c) scan order (the first maximum
wins), backward "last writer in (oh, ow) scan order".  Soft-max: A = out (t_j + sum_k out_k t_k + 1), t = |x - max| + 1 (expf of an
argument carries that argument's absolute rounding error), plus an absolute 2^-126 / (C_FACTOR 2^-24) for results that underflow.  Adam: the reference kernels' formula in float64 from the same float32
inputs, with the error of each intermediate carried through (adam_ref).
"""
import numpy as np

import convref as R

C_FACTOR, U24 = R.C_FACTOR, R.U24
APPLY_TERMS = 4   # x - mean, / sd, sd itself, the fma: roundings relative to |g x_hat|
DX_TERMS = 4
EPS = 1e-7        # the trainer's batch-norm eps (resnet_amd/trainer.py)
TINY32 = 2.0 ** -126
STEP = 16         # images per float64 block of the whole-tensor sums


# ---------------------------------------------------------------------------------------------------------------------------
# batch norm
def _c(v):
    return np.asarray(v, np.float64)[None, :, None, None]


def stats_ref(x):
    """float64 mean / biased var per channel of x [n, c, H, W] (every image of those channels) and their bounds"""
    n = x.shape[0]
    Cn = x.shape[1]
    s, s2, sa = np.zeros(Cn), np.zeros(Cn), np.zeros(Cn)
    step = STEP
    M = n * x.shape[2] * x.shape[3]
    for i in range(0, n, step):
        xc = x[i:i + step].astype(np.float64)
        s += xc.sum((0, 2, 3)); sa += np.abs(xc).sum((0, 2, 3)); s2 += (xc * xc).sum((0, 2, 3))
    mu = s / M
    var = np.zeros(Cn)
    for i in range(0, n, step):
        d = x[i:i + step].astype(np.float64) - mu[None, :, None, None]
        var += (d * d).sum((0, 2, 3))
    return mu, var / M, C_FACTOR * U24 * sa / M, C_FACTOR * U24 * s2 / M


def grad_sums(g, x, means, vars_, eps):
    """convref.bn_grad_sums over blocks of STEP images (host memory)"""
    tot = None
    for i in range(0, g.shape[0], STEP):
        part = R.bn_grad_sums(g[i:i + STEP], x[i:i + STEP], means, vars_, eps)
        tot = part if tot is None else tuple(a + b for a, b in zip(tot, part))
    return tot


def stats_violations(gm, gv, x):
    """channels of (gm, gv) outside the bounds of stats_ref(x), and the worst distance in 2^-24 (bound scale) units"""
    mu, var, bm, bv = stats_ref(x)
    em, ev = np.abs(np.asarray(gm, np.float64) - mu), np.abs(np.asarray(gv, np.float64) - var)
    bad = int(np.count_nonzero(~(em <= bm))) + int(np.count_nonzero(~(ev <= bv)))
    return bad, float(max(np.max(em / bm), np.max(ev / bv))) * C_FACTOR


def apply_ref(x, gamma, beta, means, vars_, eps, relu, residual=None):
    """ref, A of the BN apply on x [n, c, H, W] with the per-channel vectors of those channels"""
    sd = np.sqrt(np.asarray(vars_, np.float64) + eps)
    xh = (x.astype(np.float64) - _c(means)) / _c(sd)
    gx = _c(gamma) * xh
    ref = gx + _c(beta)
    A = APPLY_TERMS * np.abs(gx) + np.abs(_c(beta))
    if residual is not None:
        ref += residual
        A += np.abs(residual)
    if relu or residual is not None:
        ref = np.maximum(ref, 0.0)
    return ref, A


def bn_gate_y(x, gamma, beta, means, vars_, eps):
    """float64 y = g x_hat + b (the mode-1 gate's argument) and its bound"""
    ref, A = apply_ref(x, gamma, beta, means, vars_, eps, False)
    return ref, C_FACTOR * U24 * A


def dx_ref(g, x, gamma, means, vars_, eps, sums, M):
    """ref, A of the BN backward dx on a slab (g: gated gradient, x: the BN input, per-channel vectors of the slab's channels; sums =
    (dbeta, dgamma, sum|g|, sum|g x_hat|) of those channels in float64)"""
    db, dg, adb, adg = (np.asarray(a, np.float64) for a in sums)
    sd = np.sqrt(np.asarray(vars_, np.float64) + eps)
    xh = (x.astype(np.float64) - _c(means)) / _c(sd)
    s = _c(gamma / sd)
    k1, k2 = _c(db / M), _c(dg / M)
    g64 = g.astype(np.float64)
    ref = s * (g64 - k1 - xh * k2)
    A = np.abs(s) * (DX_TERMS * (np.abs(g64) + np.abs(k1) + np.abs(xh * k2)) + _c(adb / M) + np.abs(xh) * _c(adg / M))
    return ref, A


def bn_dx_slabs(g, x, gamma, means, vars_, eps, sums, S, Rc):
    """dx_ref on convref's two slabs: every channel of the images S, every image of the channels Rc"""
    M = x.shape[0] * x.shape[2] * x.shape[3]
    out = []
    ref, A = dx_ref(g[S], x[S], gamma, means, vars_, eps, sums, M)
    out.append(R.Slab("images %s" % (S,), ref, A, lambda a, S=S: a[S]))
    sub = [np.asarray(v)[Rc] for v in sums]
    ref, A = dx_ref(g[:, Rc], x[:, Rc], gamma[Rc], means[Rc], vars_[Rc], eps, sub, M)
    out.append(R.Slab("channels %d of %d" % (len(Rc), x.shape[1]), ref, A, lambda a, Rc=Rc: a[:, Rc]))
    return out


def bn_apply_slabs(x, gamma, beta, means, vars_, eps, relu, residual, S, Rc):
    out = []
    ref, A = apply_ref(x[S], gamma, beta, means, vars_, eps, relu, None if residual is None else residual[S])
    out.append(R.Slab("images %s" % (S,), ref, A, lambda a, S=S: a[S]))
    ref, A = apply_ref(x[:, Rc], gamma[Rc], beta[Rc], means[Rc], vars_[Rc], eps, relu, None if residual is None else residual[:, Rc])
    out.append(R.Slab("channels %d of %d" % (len(Rc), x.shape[1]), ref, A, lambda a, Rc=Rc: a[:, Rc]))
    return out


def sums_violations(db, dg, ref_sums):
    """channels of the kernel's dbeta / dgamma outside C_FACTOR 2^-24 sum|terms|, and the worst distance in 2^-24 sum|terms|"""
    rdb, rdg, adb, adg = ref_sums
    eb, eg = np.abs(np.asarray(db, np.float64) - rdb), np.abs(np.asarray(dg, np.float64) - rdg)
    bb, bg = C_FACTOR * U24 * adb, C_FACTOR * U24 * adg
    bad = int(np.count_nonzero(~((eb <= bb) | ((adb == 0) & (db == 0))))) + int(np.count_nonzero(~((eg <= bg) | ((adg == 0) & (dg == 0)))))
    w = float(max(np.max(eb / np.maximum(adb * U24, 1e-300)), np.max(eg / np.maximum(adg * U24, 1e-300))))
    return bad, w


def channel_last(y, par):
    """the channel-last copy bn_apply_cl_kernel writes of y [N, C, H, H], halos zero: one plane [N][H+2][H+2][C] with a halo of 1, or
    (par) the four parity planes [N][4][H/2+1][H/2+1][C] of a stride-2 3x3 (plane 2 (y & 1) + (x & 1), a leading zero row / column)"""
    N, Cn, H, _ = y.shape
    if not par:
        out = np.zeros((N, H + 2, H + 2, Cn), y.dtype)
        out[:, 1:H + 1, 1:H + 1] = y.transpose(0, 2, 3, 1)
        return out
    Hp = H // 2 + 1
    out = np.zeros((N, 4, Hp, Hp, Cn), y.dtype)
    for py in (0, 1):
        for px in (0, 1):
            out[:, 2 * py + px, 1:, 1:] = y[:, :, py::2, px::2].transpose(0, 2, 3, 1)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# max-pool 3x3 / stride 2 / pad 1 (even H), restated from its documented rule
def maxpool_fwd_ref(x, last_max=False):
    """values and flat arg-max indices: strict '>' from -1024 in (r, c) scan order (last_max: '>=', a mutant)"""
    N, Cn, H, _ = x.shape
    Ho = H // 2
    xp = np.full((N, Cn, H + 2, H + 2), -np.inf, np.float32)
    xp[:, :, 1:H + 1, 1:H + 1] = x
    mv = np.full((N, Cn, Ho, Ho), -1024.0, np.float32)
    mi = np.full((N, Cn, Ho, Ho), -1024, np.int32)
    base = (np.arange(N * Cn, dtype=np.int32) * np.int32(H * H)).reshape(N, Cn, 1, 1)
    o = np.arange(Ho, dtype=np.int32)
    for r in (-1, 0, 1):
        for c in (-1, 0, 1):
            cand = xp[:, :, r + 1:r + 1 + 2 * Ho:2, c + 1:c + 1 + 2 * Ho:2]
            upd = (cand >= mv) if last_max else (cand > mv)
            mv = np.where(upd, cand, mv)
            mi = np.where(upd, base + ((2 * o[:, None] + r) * H + 2 * o[None, :] + c), mi)
    return mv, mi


def maxpool_bwd_ref(idx, dy, H, first_writer=False):
    """dx[e] = dy of the LAST window in (oh, ow) scan order whose arg-max is e (first_writer: the first, a mutant).  The output index o
    grows in scan order, so the writer is the window with the largest (smallest) o among those naming e; windows of one parity class
    (oh & 1, ow & 1) are disjoint, so each class names every element at most once"""
    N, Cn, Ho, _ = dy.shape
    total = N * Cn * H * H
    pick = np.full(total, -1 if not first_writer else np.iinfo(np.int32).max, np.int32)
    o = np.arange(N * Cn * Ho * Ho, dtype=np.int32).reshape(N, Cn, Ho, Ho)
    for a in (0, 1):
        for b in (0, 1):
            cls = np.full(total, -1, np.int32)
            cls[idx[:, :, a::2, b::2].ravel()] = o[:, :, a::2, b::2].ravel()
            if first_writer:
                pick = np.where(cls >= 0, np.minimum(pick, cls), pick)
            else:
                pick = np.maximum(pick, cls)
            del cls
    if first_writer:
        pick[pick == np.iinfo(np.int32).max] = -1
    dyf = dy.ravel()
    dx = np.where(pick >= 0, dyf[np.maximum(pick, 0)], np.float32(0))
    return dx.reshape(N, Cn, H, H).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# soft-max, average pool
def softmax_ref(x):
    """float64 soft-max of the rows of x and A = out (t + sum_k out_k t_k + 1), t = |x - max| + 1"""
    x64 = x.astype(np.float64)
    mx = x64.max(1, keepdims=True)
    e = np.exp(x64 - mx)
    out = e / e.sum(1, keepdims=True)
    t = np.abs(x64 - mx) + 1.0
    # + an absolute floor: results below float32's normal range (expf of x - max < -87) may flush to 0
    return out, out * (t + (out * t).sum(1, keepdims=True) + 1.0) + TINY32 / (C_FACTOR * U24)


def softmax_f32(x, subtract_max=True):
    """a float32 execution (numpy): the valid form, or (subtract_max=False) the mutant that overflows on large logits"""
    x = x.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(x - x.max(1, keepdims=True)) if subtract_max else np.exp(x)
        return (e / e.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)


def softmax_rows(N, L, seed):
    """logits of the benchmark's scale, plus rows with |x| ~ 80-100 (where a soft-max without the max subtraction overflows or flushes to
    0 / 0) and rows with many equal maxima"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((max(N, 7), L)) * 3.0).astype(np.float32)
    x[1] += np.float32(95.0)
    x[2] -= np.float32(110.0)
    x[3] = np.float32(88.0)                                     # every entry the maximum
    x[4, rng.choice(L, 37, replace=False)] = x[4].max() + np.float32(1.0)
    x[5] = np.round(x[5])                                      # many ties, including at the maximum
    x[6, ::2] = np.float32(80.0); x[6, 1::2] = np.float32(-80.0)
    return x if N >= 7 else x[np.arange(N) * 6 // max(1, N - 1) if N > 1 else [0]].copy()  # (small N: rows spread over the planted ones)


def avgpool_ref(x):
    """float64 mean of every plane of x [N, C, H, W] and A = mean |x|"""
    x64 = x.reshape(x.shape[0], x.shape[1], -1).astype(np.float64)
    return x64.mean(2), np.abs(x64).mean(2)


# ---------------------------------------------------------------------------------------------------------------------------
# Adam (kernels_misc.hip adam_kernel = the reference's updateMeans / updateVars / updateParams)
def adam_ref(p, g, m, v, lr, wd, b1, b2, cb1, cb2, eps, bias_b=False):
    """float64 (p', m', v') of the update from float32 inputs (hyper-parameters as float32), each with A such that C_FACTOR 2^-24 A bounds
    the float32 execution: m' and v' carry |terms| (the gradient g + wd p included); p' carries |p|, |wd p|, lr |r| and what the bounds of
    m', v' carry through r = (m' / (1 - cb1)) / (sqrt(v' / (1 - cb2)) + eps).  bias_b: the mutant that corrects by b instead of b^t.
    Where g is NaN / Inf the moments stay and p' is formed from them (the reference's kernels)."""
    f = lambda a: np.float64(np.float32(a))
    lr, wd, b1, b2, cb1, cb2, eps = (f(a) for a in (lr, wd, b1, b2, cb1, cb2, eps))
    if bias_b:
        cb1, cb2 = b1, b2
    p64, g64, m64, v64 = (a.astype(np.float64) for a in (p, g, m, v))
    ok = np.isfinite(g64)
    gs = np.where(ok, g64, 0.0)
    gd = gs + wd * p64
    agd = np.abs(gs) + np.abs(wd * p64)
    m1 = np.where(ok, b1 * m64 + (1 - b1) * gd, m64)
    v1 = np.where(ok, b2 * v64 + (1 - b2) * gd * gd, v64)
    Am = np.where(ok, np.abs(b1 * m64) + (1 - b1) * agd, np.abs(m64))   # (kept moments: the tests ask for them bit for bit)
    Av = np.where(ok, b2 * v64 + (1 - b2) * agd * agd * 3, v64)
    ma, va = m1 / (1 - cb1), v1 / (1 - cb2)
    s = np.sqrt(va)
    den = s + eps
    r = ma / den
    # absolute error bounds of ma and s (2 roundings of their own each, plus the carried bounds)
    Ema = (C_FACTOR * U24 * Am + 2 * U24 * np.abs(m1)) / (1 - cb1) + 2 * U24 * np.abs(ma)
    Eva = (C_FACTOR * U24 * Av + 2 * U24 * v1) / (1 - cb2) + 2 * U24 * va
    with np.errstate(divide="ignore", invalid="ignore"):
        Es = np.where(s > 0, np.minimum(Eva / (2 * s), np.sqrt(Eva)), np.sqrt(Eva)) + U24 * s
    Er = Ema / den + np.abs(ma) * Es / (den * den) + 2 * U24 * np.abs(r)
    p1 = p64 - (lr * r + wd * p64)
    Ap = np.abs(p64) + np.abs(wd * p64) + lr * np.abs(r) + lr * Er / (C_FACTOR * U24)
    return (p1, Ap), (m1, Am), (v1, Av)


def adam_f32(p, g, m, v, lr, wd, b1, b2, cb1, cb2, eps):
    """a float32 execution (numpy) of the kernel's arithmetic, in its order"""
    f = np.float32
    lr, wd, b1, b2, cb1, cb2, eps = (f(a) for a in (lr, wd, b1, b2, cb1, cb2, eps))
    ok = np.isfinite(g)
    gd = np.where(ok, g, f(0)) + wd * p
    m1 = np.where(ok, b1 * m + (f(1) - b1) * gd, m)
    v1 = np.where(ok, b2 * v + (f(1) - b2) * gd * gd, v)
    ma, va = m1 / (f(1) - cb1), v1 / (f(1) - cb2)
    p1 = p - (lr * (ma / (np.sqrt(va) + eps)) + wd * p)
    return p1.astype(np.float32), m1.astype(np.float32), v1.astype(np.float32)


def arena_floats(dims):
    """the trainer's parameter arena: every tensor of synth.location_table padded to 64 floats (trainer.c align_up)"""
    import synth
    return sum((size + 63) // 64 * 64 for size, _, _ in synth.location_table(dims))


# ---------------------------------------------------------------------------------------------------------------------------
# the batch-norm sites of ResNet-50 (any N: the plane sizes do not depend on it).  Forward forms: "relu" (stem, reduction, spatial), "none" (projection), "add_relu"
# (expansion: + shortcut, ReLU), and in bf16 the dual writes of bn_apply_cl_kernel: "cl plane" / "cl par" (the reduction BN writes its 3x3's
# channel-last input), "cl par add_relu" (the expansion BN writes the next block's projection input as parity planes).  Backward modes
# (mid_bn_bwd_t): 1 = gate recomputed from y > 0, 3 = external mask + gated dy written, 0 = dy already gated.
# (C, H, forward forms, backward modes); storage pairs: "f32" = (f32, f32), "bf16" = (bf16, bf16), "f32>bf16" = fp32 convolution output,
# bf16 activation (the bf16 stem under RESNET_MI_BF16_STEM_TENSORS=f32)
STEM_SHAPE = (64, 112)
BN_SHAPES = [
    (64, 112, ("relu",), (1,)),
    (64, 56, ("relu", "cl plane"), (1,)),
    (256, 56, ("none", "add_relu", "cl par add_relu"), (3, 0)),
    (128, 56, ("relu", "cl par"), (1,)),
    (128, 28, ("relu", "cl plane"), (1,)),
    (512, 28, ("none", "add_relu", "cl par add_relu"), (3, 0)),
    (256, 28, ("relu", "cl par"), (1,)),
    (256, 14, ("relu", "cl plane"), (1,)),
    (1024, 14, ("none", "add_relu", "cl par add_relu"), (3, 0)),
    (512, 14, ("relu", "cl par"), (1,)),
    (512, 7, ("relu", "cl plane"), (1,)),
    (2048, 7, ("none", "add_relu"), (3, 0)),
]


FORM_ORDER = ("relu", "cl plane", "cl par", "none", "add_relu", "cl par add_relu")
MODE_ORDER = (1, 3, 0)


def bn_shapes(dims):
    """BN_SHAPES of any net: every (C, H) a batch norm of forward_pass normalises, in order of first appearance, with every forward form and
    backward mode the net's structure allows there -- the channel-last dual writes wherever a 3x3 reads the output (the reduction BN in front
    of a stride-1 / stride-2 spatial convolution, the expansion BN in front of the next block's stride-2 projection; parity planes only over
    even planes), whichever route the trainer then takes"""
    f, Hs = dims["init_conv_filters"], dims["input"] // dims["init_conv_stride"]
    forms, modes = {(f, Hs): {"relu"}}, {(f, Hs): {1}}
    bl = R.blocks(dims)

    def add(Cn, H, form, mode=None):
        forms.setdefault((Cn, H), set()).add(form)
        modes.setdefault((Cn, H), set()).update(() if mode is None else (mode,))

    for i, b in enumerate(bl):
        H, s, Ho = b["H"], b["s"], b["H"] // b["s"]
        nxt = bl[i + 1] if i + 1 < len(bl) else None
        add(b["red"], H, "relu", 1)
        if s == 1 or H % 2 == 0:
            add(b["red"], H, "cl plane" if s == 1 else "cl par")
        add(b["red"], Ho, "relu", 1)
        if b["proj"]:
            add(b["ex"], Ho, "none", 3)
        add(b["ex"], Ho, "add_relu", 0 if b["proj"] else 3)
        if nxt and nxt["proj"] and nxt["s"] == 2 and nxt["H"] % 2 == 0:
            add(b["ex"], Ho, "cl par add_relu")
    return [(Cn, H, tuple(x for x in FORM_ORDER if x in forms[(Cn, H)]), tuple(m for m in MODE_ORDER if m in modes[(Cn, H)]))
            for (Cn, H) in forms]


def _pairs(Cn, H, stem=STEM_SHAPE):
    return ("f32", "bf16", "f32>bf16") if (Cn, H) == stem else ("f32", "bf16")


def trainer_bn_fwd_cases(dims):
    """(pair, C, H, forms) over bn_shapes(dims): the channel-last forms in bf16 storage only; the stem also as "f32>bf16" """
    stem = (dims["init_conv_filters"], dims["input"] // dims["init_conv_stride"])
    out = []
    for Cn, H, forms, _ in bn_shapes(dims):
        for pr in _pairs(Cn, H, stem):
            out.append((pr, Cn, H, tuple(f for f in forms if pr == "bf16" or not f.startswith("cl"))))
    return out


def trainer_bn_bwd_cases(dims):
    """(pair, C, H, mode) over bn_shapes(dims)"""
    stem = (dims["init_conv_filters"], dims["input"] // dims["init_conv_stride"])
    return [(pr, Cn, H, mode) for Cn, H, _, modes in bn_shapes(dims) for pr in _pairs(Cn, H, stem) for mode in modes]


def bn_fwd_cases():
    """(pair, C, H, forms) of BN_SHAPES (ResNet-50): the channel-last forms in bf16 storage only"""
    out = []
    for Cn, H, forms, _ in BN_SHAPES:
        for pr in _pairs(Cn, H):
            out.append((pr, Cn, H, tuple(f for f in forms if pr == "bf16" or not f.startswith("cl"))))
    return out


def bn_bwd_cases():
    """(pair, C, H, mode)"""
    return [(pr, Cn, H, mode) for Cn, H, _, modes in BN_SHAPES for pr in _pairs(Cn, H) for mode in modes]


def trainer_bn_sites(L, dims=None, N=None):
    """every (pair, C, H, "fwd", form) and (pair, C, H, "bwd", mode) that forward_pass / backwards_pass (resnet_amd/csrc/trainer.c) produce
    for the net (default ResNet-50) at batch N (default 256) with default switches, restated from plan_layers, unit_fwd and unit_bwd; mode
    "parts" = the BN' whose reduction a fusing dgrad did (mid_bn_bwd_parts_t, the dgrad cases of convref.trainer_dgrad_bn_cases).  L: the
    library (mi_conv_plan answers the route queries)"""
    import synth
    d = dims or synth.R50_DIMS
    N = N or R.N256
    f, Hs = d["init_conv_filters"], d["input"] // d["init_conv_stride"]
    blocks = R.blocks(d)
    out = set()
    for dt in ("f32", "bf16"):
        bf = dt == "bf16"
        route = (lambda op, Cn, H, K, k, s: R.bf16_route(L, op, N, Cn, H, K, k, s)) if bf else (lambda *a: "default")
        # the stem: conv_out_dt keeps fp32 for the fp32 trainer; the bf16 trainer stores bf16, or fp32 under STEM_TENSORS=f32
        for pr in (("bf16", "f32>bf16") if bf else ("f32",)):
            out.add((pr, f, Hs, "fwd", "relu"))
            out.add((pr, f, Hs, "bwd", 1))

        def fuses(site, Cn, H, K, k, s):
            """the planner's fz (mi_layer_plan) and whether the launch fuses: fp32 site 4 only (RESNET_MI_F32_BNFUSE_BWD = 4) where the dgrad runs on the
            implicit GEMM; bf16 every site whose dgrad runs on the NCHW kernels, which fuse where the plane is a multiple of 4"""
            if not bf:  # (mi_op_conv_dgrad_bn_bwd_f32 fuses where the dgrad runs on the implicit GEMM)
                return site == 4 and R.conv_plan(L, 0, "default", "dgrad", N, Cn, H, K, k, s) is not None
            return route("dgrad", Cn, H, K, k, s) == "default" and (H * H) % 4 == 0

        for i, b in enumerate(blocks):
            H, s, Ho = b["H"], b["s"], b["H"] // b["s"]
            nxt = blocks[i + 1] if i + 1 < len(blocks) else None
            # forward: reduction (+ the 3x3's planes where B->spa.cl_by_bn), spatial, projection, expansion (+ the next projection's planes)
            form = "relu"
            if bf and route("fwd", b["red"], H, b["red"], 3, s) == "cl" and (s == 1 or H % 2 == 0):
                form = "cl plane" if s == 1 else "cl par"
            out.add((dt, b["red"], H, "fwd", form))
            out.add((dt, b["red"], Ho, "fwd", "relu"))
            if b["proj"]:
                out.add((dt, b["ex"], Ho, "fwd", "none"))
            form = "add_relu"
            if bf and nxt and nxt["proj"]:
                pk = 3 if nxt["s"] == 2 else 1
                if pk == 3 and route("fwd", nxt["inc"], nxt["H"], nxt["ex"], pk, nxt["s"]) == "cl" and nxt["H"] % 2 == 0:
                    form = "cl par add_relu"
            out.add((dt, b["ex"], Ho, "fwd", form))
            # backward: projection mode 3; expansion mode 0 after a projection, else mode 3 unless the block above's reduction dgrad
            # (site 4) did its reduction; spatial fed by the expansion dgrad (site 1), reduction by the spatial dgrad (site 2)
            if b["proj"]:
                out.add((dt, b["ex"], Ho, "bwd", 3))
                out.add((dt, b["ex"], Ho, "bwd", 0))
            elif nxt is not None and fuses(4, nxt["inc"], nxt["H"], nxt["red"], 1, 1):
                out.add((dt, b["ex"], Ho, "bwd", "parts"))
            else:
                out.add((dt, b["ex"], Ho, "bwd", 3))
            out.add((dt, b["red"], Ho, "bwd", "parts" if fuses(1, b["red"], Ho, b["ex"], 1, 1) else 1))
            out.add((dt, b["red"], H, "bwd", "parts" if fuses(2, b["red"], H, b["red"], 3, s) else 1))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# The loop turns of the batch-norm reductions (kernels_bn.hip), restated from the launchers: which turn a shape takes.
BN_SPLIT_MAX, BN_THREADS = 64, 256


def bn_nsplit(N, Cn):
    """bn_nsplit: the blocks per channel, min(ceil(2048 / C), N, 64), at least 1"""
    return max(1, min(-(-2048 // Cn), N, BN_SPLIT_MAX))


def bn_vec(pair, P):
    """bn_vec: elements per unit of the reductions -- fp32 / fp32: 4 where the plane allows it, else 1; bf16 storage on either side: 8, 4 or 1"""
    if pair == "f32":
        return 4 if P % 4 == 0 else 1
    return 8 if P % 8 == 0 else 4 if P % 4 == 0 else 1


def bn_reach(pair, Cn, H, N, in_flight=4):
    """what the blocks of bn_stats_kernel (in_flight 4) or bn_bwd_reduce_kernel (4; the external-mask modes 2) run at this shape:
    dict(nsplit, V, units = the largest block's unit count, whole = whole turns of its thread 0, remainder = units left to the remainder
    loop over all threads, crosses = a whole turn holds units of two images)"""
    P = H * H
    ns, V = bn_nsplit(N, Cn), bn_vec(pair, P)
    cnt = -(-N // ns)
    PV = P // V
    total = cnt * PV
    turn = in_flight * BN_THREADS
    # thread t takes whole turn k while k turn + t + (in_flight - 1) 256 < total
    turns_of = [max(0, -(-(total - t - (in_flight - 1) * BN_THREADS) // turn)) for t in range(BN_THREADS)]
    whole = turns_of[0]
    return dict(nsplit=ns, V=V, units=total, whole=whole, remainder=total - in_flight * sum(turns_of),
                crosses=whole > 0 and cnt > 1 and PV < turn * whole)


# (pair, C, H, N): N = 1, H = 66 -- one image per split, 1089 float4 units: a whole turn and a remainder; C = 2048, H = 48 -- one split, a
# whole turn that crosses from one image into the next (bf16: 8 elements per unit, so N = 4 for 1152 units); C = 2048, H = 7, N = 21 -- 1029
# scalar units, the V == 1 whole turn; C = 64, H = 4, N = 33 -- 32 splits (finalize lanes 16 .. 31), the first with two images
LOOP_TURN_SHAPES = [("f32", 64, 66, 1), ("bf16", 64, 66, 1), ("f32", 2048, 48, 2), ("bf16", 2048, 48, 4), ("f32", 2048, 7, 21),
                    ("bf16", 2048, 7, 21), ("f32", 64, 4, 33), ("bf16", 64, 4, 33)]



# ---------------------------------------------------------------------------------------------------------------------------
# soft-max / loss head: rows whose maximum a lane meets only after its first turn
DOMINANT_L = (65, 1000, 1537)
DOMINANT_GAP = 95.0   # > 89: expf of the gap overflows float32


def dominant_columns(L):
    """per row of dominant_rows(L) the column of its dominant logit: the first column past a lane's first turn, the last column, one of the
    last register slot of loss_head_kernel<reg> (960 .. 1023) where the row has it, and a row without a dominant logit (-1)"""
    cols = [64, L - 1, min(L - 1, 64 + (L - 65) // 2)]
    if L > 960:
        cols.append(min(L - 1, 990))
    return cols + [-1]


def dominant_rows(L, seed=73):
    """N(0, 9) logits; row r has x[r, dominant_columns(L)[r]] = max of the row + DOMINANT_GAP"""
    cols = dominant_columns(L)
    rng = np.random.default_rng(seed + L)
    x = (rng.standard_normal((len(cols), L)) * 3.0).astype(np.float32)
    for r, c in enumerate(cols):
        if c >= 0:
            x[r, c] = x[r].max() + np.float32(DOMINANT_GAP)
    return x


ADAM_GRID_CAP = 16384   # ew_blocks (kernels_misc.hip): workgroups of 256 threads; a thread takes a second turn past 16384 x 256 elements


def adam_second_turn_inputs():
    """((p, g, m, v), indices of the planted NaN / Inf gradients, hyper-parameters) of test_gpu_ops.py::test_adam_second_grid_stride_turn:
    n = 16384 x 256 + 257, step 500 (1 - b1^t = 1, 1 - b2^t = 0.39), wd 5e-4; non-finite gradients in the first turn and in the second"""
    n = ADAM_GRID_CAP * 256 + 257
    rng = np.random.default_rng(83)
    p = rng.standard_normal(n, dtype=np.float32) * np.float32(0.05)
    g = rng.standard_normal(n, dtype=np.float32) * np.exp(rng.uniform(-8, 2, n)).astype(np.float32)
    m = rng.standard_normal(n, dtype=np.float32) * np.float32(1e-2)
    v = np.abs(rng.standard_normal(n, dtype=np.float32)) * np.float32(1e-4)
    bad_g = np.array([3, 12345, ADAM_GRID_CAP * 256, ADAM_GRID_CAP * 256 + 200, n - 1])
    g[bad_g] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    cb1 = cb2 = np.float32(1)
    for _ in range(500):
        cb1, cb2 = np.float32(cb1 * np.float32(0.9)), np.float32(cb2 * np.float32(0.999))
    return (p, g, m, v), bad_g, dict(lr=1e-3, wd=5e-4, b1=0.9, b2=0.999, cb1=cb1, cb2=cb2, eps=1e-7)


def adam_violations(got, inputs, hp, first=0):
    """elements of got = (p', m', v') outside the bounds of adam_ref on inputs = (p, g, m, v), in blocks (host memory), and the worst
    distance; first: the index the comparison starts at"""
    p, g, m, v = inputs
    bad, worst = 0, 0.0
    for i in range(first, p.size, 1 << 21):
        sl = slice(i, i + (1 << 21))
        for a, (ref, A) in zip(got, adam_ref(p[sl], g[sl], m[sl], v[sl], **hp)):
            w, b = R.dist_f32(a[sl], ref, A)
            bad, worst = bad + b, max(worst, w)
    return bad, worst


def dominant_labels(L):
    """labels for dominant_rows(L): the dominant column, a column past 63 that is not it, column 0, ... -- every row's label is valid and
    some lie past column 63"""
    cols = dominant_columns(L)
    lab = [cols[0], 64 if L > 65 else 0, 0] + [cols[3]] * (len(cols) - 4) + [L - 1]
    return np.asarray(lab[:len(cols)], np.int32)
