"""The per-element GPU checks of test_gpu_batch256.py, test_gpu_batch256_ew.py and test_gpu_ragged.py: each function runs one operator at
batch N on one case of the lists convref / ewref build and checks it against the float64 reference with the bounds of convref (fp32
outputs |got - ref| <= 64 * 2^-24 * A, bf16 outputs between RNE(ref -/+ that bound), statistics and BN' sums to 64 * 2^-24 * sum |terms|,
bit for bit where the operation is exact).  `record(key, worst)` collects the worst distance per key for the module's summary.

Every body comes in two halves: `<name>_inputs` builds a case's operands and `<name>_call` runs the operator on them (no reference: what
test_gpu_redzone.py runs under the allocator's red-zone mode); `<name>` itself calls both and checks the result.  `gen` / `cheap` swap
the Gaussian operands for `pattern`, a cheap deterministic one, where only the run matters."""
import time

import numpy as np

import convref as R
import ewref as E
import synth

EPS = E.EPS
F = np.float32
F32, BF16 = 0, 1
PAIRS = {"f32": (F32, F32), "bf16": (BF16, BF16), "f32>bf16": (F32, BF16)}


def normal(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * np.float32(scale))


def pattern(shape, seed, scale=1.0):
    """a cheap deterministic operand in place of normal(): the 17 values -1, -7/8, ..., 1 (bf16 numbers) in a sequence of period 251"""
    base = (((np.arange(251) * 7 + seed) % 17 - 8) / 8.0).astype(F) * F(scale)
    return np.resize(base, int(np.prod(shape))).reshape(shape)


def _rnd_bf(bf):
    return R.bf16_round32 if bf else (lambda a: a)


def _wscale(Cn, K, k):
    return (2.0 / (k * k * (Cn + K))) ** 0.5


# ---------------------------------------------------------------------------------------------------------------------------
# convolutions
def _conv_seed(case):
    return hash(tuple(case[3:8])) % 1000


def conv_route_inputs(case, N, gen=normal):
    """the operands of one conv_route case: w, and x / dy / addend as the op takes them"""
    dt, route, op, Cn, H, K, k, s, where = case
    Ho = H // s
    rnd = _rnd_bf(dt == "bf16")
    seed = _conv_seed(case)
    inp = dict(w=rnd(gen((K, Cn, k, k), seed + 1, _wscale(Cn, K, k))), x=None, dy=None, addend=None)
    if op != "dgrad":
        inp["x"] = rnd(gen((N, Cn, H, H), seed + 2))
    if op != "fwd":
        inp["dy"] = rnd(gen((N, K, Ho, Ho), seed + 3))
    if op == "dgrad" and "red" in where:
        inp["addend"] = rnd(gen((N, Cn, H, H), seed + 4))
    return inp


def conv_route_call(ops, case, inp):
    """the case's operator on its route; returns its one output"""
    dt, route, op, Cn, H, K, k, s, where = case
    bf = dt == "bf16"
    x, w, dy, addend = inp["x"], inp["w"], inp["dy"], inp["addend"]
    if op == "fwd":
        if route == "default":
            return ops.conv_fwd_bf16(x, w, s) if bf else ops.conv_fwd(x, w, s)
        if route == "cl":
            return ops.conv_fwd_bf16_cl(x, w, s)
        return ops.conv1x1_fwd_bf16_cl(x, w)
    if op == "dgrad":
        if route == "default":
            return ops.conv_dgrad_bf16(w, dy, H, s, dx_init=addend) if bf else ops.conv_dgrad(w, dy, H, s, dx_init=addend)
        return ops.conv_dgrad_bf16_cl(w, dy, H, dx_init=addend, stride=s)
    if route == "default" or route == "pw":
        return ops.conv_wgrad_bf16(x, dy, k, s) if bf else ops.conv_wgrad(x, dy, k, s)
    if route == "cl":
        return ops.conv_wgrad_bf16_cl(x, dy, s)
    return ops.conv_wgrad_bf16_cl2(x, dy, s)


def conv_route(ops, case, N, record):
    """one (dtype, route, op) of a layer on the slabs; the FC-free half of test_gpu_batch256.py"""
    dt, route, op, Cn, H, K, k, s, where = case
    bf = dt == "bf16"
    Ho = H // s
    L = ops.L
    plan = R.conv_plan(L, 1 if bf else 0, route, op, N, Cn, H, K, k, s)
    assert plan is not None or (not bf and route == "default"), "%s refuses %s" % (route, case)
    seed = _conv_seed(case)
    inp = conv_route_inputs(case, N)
    x, w, dy, addend = inp["x"], inp["w"], inp["dy"], inp["addend"]
    t0 = time.time()
    got = conv_route_call(ops, case, inp)
    if op == "fwd":
        Pc = (Ho * Ho + 7) // 8 * 8 if bf and route == "default" else Ho * Ho
        S = R.slab_images(N, plan, K, Pc, seed)
        slabs = R.fwd_slabs(x, w, s, S, R.slab_channels(K, seed))
    elif op == "dgrad":
        Pc = (H * H + 7) // 8 * 8 if bf and route == "default" else H * H
        S = R.slab_images(N, plan, Cn, Pc, seed)
        slabs = R.dgrad_slabs(w, dy, H, s, S, R.slab_channels(Cn, seed), addend)
    else:
        slabs = R.wgrad_slabs(x, dy, k, s, R.slab_channels(K, seed), R.slab_channels(Cn, seed + 1))
    # the weight gradient is fp32 on every route; fwd / dgrad outputs are stored as bf16 on the bf16 routes
    out_bf = bf and op != "wgrad"
    t1 = time.time()
    worst = R.check_slabs(got, slabs, out_bf, "%s %s %s %s" % (dt, route, op, (Cn, H, K, k, s)))
    record((dt, route, op), worst)
    print("%s plan %s: worst %.3g %s (kernel, transfers and reference %.1f s, check %.1f s)"
          % (case, plan, worst, "bf16 ulp" if out_bf else "x 2^-24 A", t1 - t0, time.time() - t1))


def fc_gemm_inputs(form, N, Dn, Ln, gen=normal):
    """(a, b) of the product `form`"""
    X = np.maximum(gen((N, Dn), 31), 0)  # pooled ReLU features
    W = gen((Dn, Ln), 32, 0.01)
    dY = gen((N, Ln), 33)
    return {"nn": (X, W), "lt": (X, dY), "rt": (dY, W)}[form]


def fc_gemm_call(ops, form, inp):
    return ops.matmul(inp[0], inp[1], form)


def fc_gemm(ops, form, N, Dn, Ln, record):
    """the FC layer's three products at N x Dn x Ln: logits = X W, dW = X^T dY, dX = dY W^T (full float64 reference)"""
    a, b = inp = fc_gemm_inputs(form, N, Dn, Ln)
    got = fc_gemm_call(ops, form, inp)
    if form == "nn":
        ref, A = a.astype(np.float64) @ b, np.abs(a).astype(np.float64) @ np.abs(b)
    elif form == "lt":
        ref, A = a.T.astype(np.float64) @ b, np.abs(a.T).astype(np.float64) @ np.abs(b)
    else:
        ref, A = a.astype(np.float64) @ b.T, np.abs(a).astype(np.float64) @ np.abs(b.T)
    worst, bad = R.dist_f32(got, ref, A)
    assert bad == 0, "FC %s: %d elements out of bounds (worst %.3g x 2^-24 A)" % (form, bad, worst)
    record(("f32", "fc", form), worst)


def _stem_data(N, H, bf, gen=normal):
    rnd = _rnd_bf(bf)
    x = rnd(gen((N, 3, H, H), 41, 60.0))                          # images of the scale the batch source gives (about +-124)
    w = rnd(gen((64, 3, 7, 7), 42, _wscale(3, 64, 7)))
    return x, w


def stem_inputs(dt, op, N, H, gen=normal):
    bf = dt == "bf16"
    x, w = _stem_data(N, H, bf, gen)
    return dict(x=x, w=w, dy=_rnd_bf(bf)(gen((N, 64, H // 2, H // 2), 43)) if op != "fwd" else None)


def stem_call(ops, dt, op, inp, dy_dt=F32):
    bf = dt == "bf16"
    x, w, dy = inp["x"], inp["w"], inp["dy"]
    if op == "fwd":
        return ops.stem_fwd_bf16(x, w, exact=not bf)
    return ops.stem_wgrad_bf16_t(x, w, dy, dy_dt) if dy_dt == BF16 else ops.stem_wgrad_bf16(x, w, dy, exact=not bf)


def stem(ops, dt, op, N, H, record, dy_dt=F32):
    """the 7x7 stride-2 stem on its matrix-core kernels (exact fp32, or bf16 operands with fp32 accumulation; fp32 tensors, or with dy_dt =
    BF16 the bf16 trainer's bf16 dY): the forward on the slabs, the weight gradient against the full float64 reduction over every image"""
    inp = stem_inputs(dt, op, N, H)
    x, w, dy = inp["x"], inp["w"], inp["dy"]
    got = stem_call(ops, dt, op, inp, dy_dt)
    if op == "fwd":
        slabs = R.fwd_slabs(x, w, 2, R.slab_images(N, seed=7), R.slab_channels(64, 7))
    else:
        slabs = R.wgrad_slabs(x, dy, 7, 2, list(range(64)), [])     # every row: the whole weight gradient
    worst = R.check_slabs(got, slabs, False, "stem %s %s" % (dt, op))
    record((dt, "stem", op + (" bf16 dy" if dy_dt == BF16 else "")), worst)
    print("stem %s %s: worst %.3g x 2^-24 A" % (dt, op, worst))


def bn_params_conv(Cn, seed, gen=normal):
    gamma = (1 + 0.2 * gen((Cn,), seed)).astype(np.float32)
    beta = (0.3 * gen((Cn,), seed + 1)).astype(np.float32)
    return gamma, beta


def _conv_bn_check(conv, gm, gv, y, slabs, S, Rk, gamma, beta, conv_bf, y_bf, key, what, record):
    """the convolution output on the slabs; the means and variances of the channels in Rk against the float64 statistics of the exact
    convolution over all images (contract: statistics of the fp32 accumulators, before any rounding); y against the float64 apply of the
    stored convolution output with the statistics the epilogue produced.  Returns (conv, statistics, y) worst distances"""
    worst = R.check_slabs(conv, slabs, conv_bf, "%s conv" % what)
    record(key, worst)
    bad, ws = R.conv_stats_violations(gm[Rk], gv[Rk], slabs[1].ref, slabs[1].A)
    assert bad == 0, "%s statistics: %d values of %d channels out of bounds, worst %.3g x 2^-24 (bound scale)" % (what, bad, len(Rk), ws)
    record((key[0], "bn stats", key[1] + " " + key[2]), ws)
    wy = R.check_slabs(y, E.bn_apply_slabs(conv, gamma, beta, gm, gv, 1e-7, True, None, S, Rk), y_bf, "%s y" % what)
    record((key[0], "bn apply", key[1] + " " + key[2]), wy)
    return worst, ws, wy


def conv_bn_fwd_inputs(case, N, gen=normal):
    dt, Cn, H, K, k, s, where = case
    rnd = _rnd_bf(dt == "bf16")
    seed = hash((Cn, H, K, k, s)) % 1000 + 500
    x = rnd(gen((N, Cn, H, H), seed + 2))
    w = rnd(gen((K, Cn, k, k), seed + 1, _wscale(Cn, K, k)))
    gamma, beta = bn_params_conv(K, seed + 3, gen)
    return dict(x=x, w=w, gamma=gamma, beta=beta)


def conv_bn_fwd_call(ops, case, inp, route="default"):
    """returns (conv, means, vars, y, fused)"""
    dt, Cn, H, K, k, s, where = case
    x, w, gamma, beta = inp["x"], inp["w"], inp["gamma"], inp["beta"]
    if route == "cl":
        return ops.conv_bn_fwd_bf16_cl(x, w, gamma, beta, s, 1e-7, 1)
    return ops.conv_bn_fwd_t(x, w, gamma, beta, s, 1e-7, 1, 1 if dt == "bf16" else 0)


def conv_bn_fwd(ops, case, N, record, route="default"):
    """mi_op_conv_bn_fwd_t (route "default": the implicit GEMM / bf16 NCHW kernels) or mi_op_conv_bn_fwd_bf16_cl (route "cl", bf16) as
    forward_pass pairs a convolution with its BN: the statistics come from the convolution's epilogue (including the partial rows the
    sliced tail tiles and the partial last column tile write).  Every case must fuse: the trainer relies on the epilogue statistics"""
    dt, Cn, H, K, k, s, where = case
    bf = dt == "bf16"
    seed = hash((Cn, H, K, k, s)) % 1000 + 500
    inp = conv_bn_fwd_inputs(case, N)
    x, w, gamma, beta = inp["x"], inp["w"], inp["gamma"], inp["beta"]
    conv, gm, gv, y, fused = conv_bn_fwd_call(ops, case, inp, route)
    assert fused, "every layer tiles: the statistics must come from the convolution's epilogue"
    plan = R.conv_plan(ops.L, 1 if bf else 0, route, "fwd", N, Cn, H, K, k, s)
    Ho = H // s
    Pc = (Ho * Ho + 7) // 8 * 8 if bf and route == "default" else Ho * Ho
    Rk, S = R.slab_channels(K, seed), R.slab_images(N, plan, K, Pc, seed)
    slabs = R.fwd_slabs(x, w, s, S, Rk)
    w3 = _conv_bn_check(conv, gm, gv, y, slabs, S, Rk, gamma, beta, bf, bf, (dt, route, "fwd+bn"), "conv_bn %s %s %s" % (dt, route, (Cn, H, K, k, s)), record)
    print("%s %s plan %s: conv worst %.3g, statistics worst %.3g x 2^-24 (bound scale), y worst %.3g" % ((case, route, plan) + w3))


STEM_BN = {"f32": (F32, F32, True), "bf16": (F32, BF16, False), "bf16 bf16-out": (BF16, BF16, False)}  # (conv_dt, a_dt, exact)


def stem_bn_fwd_inputs(variant, N, H, gen=normal):
    conv_dt, a_dt, exact = STEM_BN[variant]
    x, w = _stem_data(N, H, not exact, gen)
    gamma, beta = bn_params_conv(64, 45, gen)
    return dict(x=x, w=w, gamma=gamma, beta=beta)


def stem_bn_fwd_call(ops, variant, inp):
    """returns (conv, means, vars, y, fused)"""
    conv_dt, a_dt, exact = STEM_BN[variant]
    return ops.stem_bn_fwd_t(inp["x"], inp["w"], inp["gamma"], inp["beta"], 1e-7, conv_dt, a_dt, exact)


def stem_bn_fwd(ops, variant, N, H, record):
    """mi_op_stem_bn_fwd_t as forward_pass runs the stem: MI_FWD_STEM_F32 ("f32"), MI_FWD_STEM_BF16 with the convolution output stored fp32
    ("bf16", RESNET_MI_BF16_STEM_TENSORS=f32) or bf16 ("bf16 bf16-out", the default: mi_trainer_stem_dtype); statistics from the stem
    kernel's partials"""
    conv_dt, a_dt, exact = STEM_BN[variant]
    inp = stem_bn_fwd_inputs(variant, N, H)
    x, w, gamma, beta = inp["x"], inp["w"], inp["gamma"], inp["beta"]
    conv, gm, gv, y, fused = stem_bn_fwd_call(ops, variant, inp)
    assert fused, "the stem's statistics must come from its kernel's partials"
    Rk, S = R.slab_channels(64, 7), R.slab_images(N, seed=7)
    slabs = R.fwd_slabs(x, w, 2, S, Rk)
    w3 = _conv_bn_check(conv, gm, gv, y, slabs, S, Rk, gamma, beta, conv_dt == BF16, a_dt == BF16, ("bf16" if not exact else "f32", "stem+bn", variant),
                        "stem_bn %s" % variant, record)
    print("stem + BN %s: conv worst %.3g, statistics worst %.3g x 2^-24 (bound scale), y worst %.3g" % ((variant,) + w3))


SMALL_VAR_EVERY, SMALL_VAR_SCALE = 8, 2e-4


def dgrad_bn_bwd_inputs(case, N, gen=normal, small_var=False):
    """small_var: every 8th channel of the normalised tensor varies by 1.5 x 2e-4 about 0.3 -- a variance of 9e-8, the size of eps (in
    bf16 storage the channel keeps two or three levels about 0.3: a variance of about 7e-7)"""
    dt, Cn, H, K, k, s, where = case
    rnd = _rnd_bf(dt == "bf16")
    seed = hash((Cn, H, K, k, s)) % 1000 + 700
    eps = 1e-7
    w = rnd(gen((K, Cn, k, k), seed + 1, _wscale(Cn, K, k)))
    dy = rnd(gen((N, K, H // s, H // s), seed + 2))
    addend = rnd(gen((N, Cn, H, H), seed + 3)) if "red" in where else None
    bn_x = gen((N, Cn, H, H), seed + 4, 1.5)
    if small_var:
        bn_x[:, ::SMALL_VAR_EVERY] *= np.float32(SMALL_VAR_SCALE)
    bn_x = rnd(bn_x + np.float32(0.3))    # the convolution output the batch norm normalised
    gamma, beta = bn_params_conv(Cn, seed + 5, gen)
    means = bn_x.mean((0, 2, 3), dtype=np.float64).astype(np.float32)
    vars_ = bn_x.var((0, 2, 3), dtype=np.float64).astype(np.float32)
    sd = np.sqrt(vars_ + np.float32(eps))
    mask = rnd(np.maximum(gamma[None, :, None, None] * ((bn_x - means[None, :, None, None]) / sd[None, :, None, None]) + beta[None, :, None, None], 0))
    return dict(w=w, dy=dy, addend=addend, bn_x=bn_x, gamma=gamma, beta=beta, means=means, vars_=vars_, mask=mask, eps=eps)


def dgrad_bn_bwd_call(ops, case, inp):
    """returns (gated, bn dx, dgamma, dbeta, fused)"""
    dt, Cn, H, K, k, s, where = case
    fn = ops.conv_dgrad_bn_bwd_bf16 if dt == "bf16" else ops.conv_dgrad_bn_bwd_f32
    return fn(inp["w"], inp["dy"], H, s, inp["bn_x"], inp["mask"], inp["gamma"], inp["beta"], inp["means"], inp["vars_"], inp["eps"],
              addend=inp["addend"])


def dgrad_bn_bwd(ops, case, N, record, small_var=False):
    """mi_op_conv_dgrad_bn_bwd_{f32,bf16} at the trainer's BN'-fusion sites: the gated dgrad (mask > 0 ? dgrad (+ addend) : 0) on the
    slabs against the convolution reference; dbeta and dgamma against float64 sums of the product's own gated output as it is stored
    (the kernels' contract: kernels_igemm_bf16.hip sums the rounded gradient), to C_FACTOR 2^-24 sum |terms|"""
    dt, Cn, H, K, k, s, where = case
    bf = dt == "bf16"
    seed = hash((Cn, H, K, k, s)) % 1000 + 700
    inp = dgrad_bn_bwd_inputs(case, N, small_var=small_var)
    w, dy, addend, bn_x, gamma, means, vars_, mask, eps = (inp[n] for n in ("w", "dy", "addend", "bn_x", "gamma", "means", "vars_", "mask", "eps"))
    gated, bdx, dg, db, fused = dgrad_bn_bwd_call(ops, case, inp)
    plan = R.conv_plan(ops.L, 1 if bf else 0, "default", "dgrad", N, Cn, H, K, k, s)
    assert fused == ((H * H) % 4 == 0 if bf else plan is not None), "which launches fuse the BN' reduction"
    Pc = (H * H + 7) // 8 * 8 if bf else H * H
    S, Rc = R.slab_images(N, plan, Cn, Pc, seed), R.slab_channels(Cn, seed)
    slabs = R.gate_slabs(R.dgrad_slabs(w, dy, H, s, S, Rc, addend), mask)
    worst = R.check_slabs(gated, slabs, bf, "gated dgrad %s %s" % (dt, (Cn, H, K, k, s)))
    record((dt, "default", "dgrad+bn'"), worst)
    rdb, rdg, adb, adg = R.bn_grad_sums(gated, bn_x, means, vars_, eps)
    eb, eg = np.abs(db - rdb), np.abs(dg - rdg)
    bb, bg = R.C_FACTOR * R.U24 * adb, R.C_FACTOR * R.U24 * adg
    assert np.all((eb <= bb) | ((adb == 0) & (db == 0))), "dbeta: %d of %d channels out of bounds" % (np.sum(eb > bb), Cn)
    assert np.all((eg <= bg) | ((adg == 0) & (dg == 0))), "dgamma: %d of %d channels out of bounds" % (np.sum(eg > bg), Cn)
    ws = float(max(np.max(eb / np.maximum(adb * R.U24, 1e-300)), np.max(eg / np.maximum(adg * R.U24, 1e-300))))
    record((dt, "bn' sums", "bwd"), ws)
    # BN' dx (mid_bn_bwd_parts_t where fused: the merged partials, then bn_bwd_apply_kernel) against the float64 formula from the sums
    wx = R.check_slabs(bdx, E.bn_dx_slabs(gated, bn_x, gamma, means, vars_, eps, (rdb, rdg, adb, adg), S, Rc), bf, "BN' dx %s %s" % (dt, (Cn, H, K, k, s)))
    record((dt, "bn' dx", "bwd"), wx)
    print("%s plan %s fused %s: gated worst %.3g %s, dbeta / dgamma worst %.3g x 2^-24 sum|terms|, dx worst %.3g"
          % (case, plan, fused, worst, "bf16 ulp" if bf else "x 2^-24 A", ws, wx))


# ---------------------------------------------------------------------------------------------------------------------------
# the element-wise half
def _rnd(dt):
    return R.bf16_round32 if dt == BF16 else (lambda a: a)


def _round_(a, dt):
    """round a to bf16 in place, a few images at a time (host memory)"""
    if dt == BF16:
        for i in range(0, a.shape[0], 16):
            a[i:i + 16] = R.bf16_round32(a[i:i + 16])
    return a


def conv_out(N, Cn, H, seed, dt):
    """a convolution output: per-channel scales 1e-3 .. 3 (small variances make eps matter) and offsets of up to 2 standard deviations"""
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(3.0), Cn)).astype(F)
    off = (rng.uniform(-2, 2, Cn) * scale).astype(F)
    x = rng.standard_normal((N, Cn, H, H), dtype=F)
    x *= scale[None, :, None, None]
    x += off[None, :, None, None]
    return _round_(x, dt)


def bn_params(Cn, seed):
    rng = np.random.default_rng(seed)
    gamma = (1 + 0.3 * np.clip(rng.standard_normal(Cn), -2.5, 2.5)).astype(F)
    beta = (0.3 * rng.standard_normal(Cn)).astype(F)
    beta[::4] = 0
    return gamma, beta


def relu_normal(shape, seed, dt):
    x = np.random.default_rng(seed).standard_normal(shape, dtype=F)
    np.maximum(x, 0, out=x)
    return _round_(x, dt)


def bn_fwd_inputs(case, N, cheap=False):
    """x, gamma, beta and the residual of the add_relu forms"""
    pair, Cn, H, forms = case
    x_dt, a_dt = PAIRS[pair]
    seed = Cn * 7 + H + 11 * x_dt + 13 * a_dt
    if cheap:
        x = _round_(pattern((N, Cn, H, H), seed, 2.0), x_dt)
        gamma, beta = bn_params_conv(Cn, seed + 1, pattern)
    else:
        x = conv_out(N, Cn, H, seed, x_dt)
        gamma, beta = bn_params(Cn, seed + 1)
    res = None
    if any("add_relu" in form for form in forms):
        res = _round_(np.maximum(pattern(x.shape, seed + 2), 0), a_dt) if cheap else relu_normal(x.shape, seed + 2, a_dt)
    return dict(x=x, gamma=gamma, beta=beta, res=res)


def bn_fwd_call(ops, case, inp, form):
    """one apply form of the case: (means, vars, y), with the channel-last copy behind them for the cl forms"""
    pair, Cn, H, forms = case
    x_dt, a_dt = PAIRS[pair]
    res = inp["res"] if "add_relu" in form else None
    if form.startswith("cl"):
        return ops.bn_fwd_cl_bf16(inp["x"], inp["gamma"], inp["beta"], EPS, residual=res, par="par" in form)
    return ops.bn_fwd_t(inp["x"], inp["gamma"], inp["beta"], EPS, form != "none", x_dt, a_dt, residual=res)


def bn_apply_call(ops, case, inp, means, vars_):
    """RECOMPUTE_BN's apply (+ ReLU) from given statistics"""
    x_dt, a_dt = PAIRS[case[0]]
    return ops.bn_apply_t(inp["x"], inp["gamma"], inp["beta"], means, vars_, EPS, 1, x_dt, a_dt)


def bn_fwd(ops, case, N, record):
    """statistics (bn_stats -> bn_finalize) per channel against float64 over all N * P samples; every apply form of this shape against the
    float64 apply with the kernel's statistics; RECOMPUTE_BN's apply from given statistics; the channel-last copies bit for bit"""
    pair, Cn, H, forms = case
    x_dt, a_dt = PAIRS[pair]
    seed = Cn * 7 + H + 11 * x_dt + 13 * a_dt
    inp = bn_fwd_inputs(case, N)
    x, gamma, beta = inp["x"], inp["gamma"], inp["beta"]
    S, Rc = R.slab_images(N, seed=seed), R.slab_channels(Cn, seed)
    abf = a_dt == BF16
    t0 = time.time()
    gm = gv = None
    for form in forms:
        res = inp["res"] if "add_relu" in form else None
        relu = form != "none"
        if form.startswith("cl"):
            m, v, y, ycl = bn_fwd_call(ops, case, inp, form)
            exp = E.channel_last(y, "par" in form)
            assert ycl.shape == exp.shape
            assert np.array_equal(ycl.view(np.uint32), exp.view(np.uint32)), \
                "%s: the channel-last copy differs from the NCHW output (or a halo is not zero) at %d elements" % (form, np.count_nonzero(ycl != exp))
            del ycl, exp
        else:
            m, v, y = bn_fwd_call(ops, case, inp, form)
        if gm is None:
            gm, gv = m, v
            bad, ws = E.stats_violations(gm[Rc], gv[Rc], x[:, Rc])
            assert bad == 0, "%s statistics: %d values out of bounds (worst %.3g x 2^-24)" % (pair, bad, ws)
            record(("bn stats " + pair, "fwd"), ws)
        else:
            assert np.array_equal(m, gm) and np.array_equal(v, gv), "%s: the statistics of one tensor differ between launches" % form
        slabs = E.bn_apply_slabs(x, gamma, beta, gm, gv, EPS, relu, res, S, Rc)
        record(("bn apply " + pair, form), R.check_slabs(y, slabs, abf, "%s %s %s" % (pair, (Cn, H), form)))
        if form == "relu":  # RECOMPUTE_BN: the same activation from the stored statistics
            y2 = bn_apply_call(ops, case, inp, gm, gv)
            assert np.array_equal(y2.view(np.uint32), y.view(np.uint32)), "RECOMPUTE_BN's apply differs from the forward's"
            del y2
        del y, res
    print("%s: %s %.1f s" % (case, forms, time.time() - t0))


def _nudge(x, gamma, beta, means, vars_, x_dt, exact0):
    """mode 1: move x away from the gate's edge wherever |y| lies within twice its bound of 0 (the elements planted at x == mean in beta == 0
    channels stay: y == 0 exactly there, in any arithmetic); returns the gate y > 0"""
    n = E.STEP
    on = np.empty(x.shape, bool)
    moved = 0
    for i in range(0, x.shape[0], n):
        sl = slice(i, i + n)
        y, b = E.bn_gate_y(x[sl], gamma, beta, means, vars_, EPS)
        amb = (np.abs(y) <= 2 * b) & ~exact0[sl]
        if amb.any():
            sd = np.sqrt(vars_.astype(np.float64) + EPS)
            sign = np.where(y >= 0, 1.0, -1.0)
            c = np.nonzero(amb)[1]
            xh = (sign[amb] * 0.25 * np.abs(gamma[c]) - beta[c]) / gamma[c]
            xs = x[sl]
            xs[amb] = _rnd(x_dt)((means[c] + sd[c] * xh).astype(F))
            moved += int(amb.sum())
            y, b = E.bn_gate_y(xs, gamma, beta, means, vars_, EPS)
            assert not np.any((np.abs(y) <= 2 * b) & ~exact0[sl]), "an element stays at the gate's edge"
        on[sl] = y > 0
    return on, moved


def bn_bwd_inputs(case, N, cheap=False):
    """x, gamma, beta, the given statistics, dy, mode 3's mask, and `on` = the gate the reference takes (None: no gate).  cheap: no planted
    or nudged elements in mode 1 (those serve the reference's gate), `on` is not computed there"""
    pair, Cn, H, mode = case
    x_dt, a_dt = PAIRS[pair]
    seed = Cn * 5 + H + 17 * mode + 11 * x_dt + 13 * a_dt + 3000
    if cheap:
        x = _round_(pattern((N, Cn, H, H), seed, 2.0), x_dt)
        gamma, beta = bn_params_conv(Cn, seed + 1, pattern)
        mu, var = x.mean((0, 2, 3), dtype=np.float64), x.var((0, 2, 3), dtype=np.float64)
        dy = _round_(pattern(x.shape, seed + 2), a_dt)
    else:
        x = conv_out(N, Cn, H, seed, x_dt)
        gamma, beta = bn_params(Cn, seed + 1)
        mu, var = E.stats_ref(x)[:2]
    means, vars_ = R.bf16_round32(mu.astype(F)), var.astype(F)
    if not cheap:
        rng = np.random.default_rng(seed + 2)
        dy = rng.standard_normal(x.shape, dtype=F)
        dy += rng.uniform(-0.5, 0.5, Cn).astype(F)[None, :, None, None]    # channel means of dy: k1 is not negligible
        _round_(dy, a_dt)
    mask = on = None
    if mode == 1 and not cheap:
        exact0 = np.zeros(x.shape, bool)
        exact0[:, ::4, ::5, ::3] = True                                   # beta == 0 in every 4th channel
        x[exact0] = np.broadcast_to(means[None, :, None, None], x.shape)[exact0]
        on, moved = _nudge(x, gamma, beta, means, vars_, x_dt, exact0)
        assert not np.any(on & exact0)
        del exact0
    elif mode == 3:
        mask = _round_(np.maximum(pattern(x.shape, seed + 3), 0), a_dt) if cheap else relu_normal(x.shape, seed + 3, a_dt)
        on = mask > 0
    return dict(x=x, gamma=gamma, beta=beta, means=means, vars_=vars_, dy=dy, mask=mask, on=on)


def bn_bwd_call(ops, case, inp):
    """returns (dx, dgamma, dbeta), with the gated dy behind them in mode 3"""
    pair, Cn, H, mode = case
    x_dt, a_dt = PAIRS[pair]
    return ops.bn_bwd_t(inp["x"], inp["gamma"], inp["beta"], inp["means"], inp["vars_"], inp["dy"], EPS, mode, x_dt, a_dt, mask_src=inp["mask"])


def bn_bwd(ops, case, N, record):
    """mi_op_bn_bwd_t: dbeta, dgamma to C_FACTOR 2^-24 sum|terms| against float64 sums of the gated gradient; dx against the float64
    formula from those sums; mode 3's gated dy bit for bit (mask > 0 ? dy : 0).  The statistics are given, as the trainer gives the stored
    ones; means are bf16 numbers so that x == mean can be planted in either storage type"""
    pair, Cn, H, mode = case
    x_dt, a_dt = PAIRS[pair]
    seed = Cn * 5 + H + 17 * mode + 11 * x_dt + 13 * a_dt + 3000
    inp = bn_bwd_inputs(case, N)
    t0 = time.time()
    res = bn_bwd_call(ops, case, inp)
    x, gamma, means, vars_ = inp["x"], inp["gamma"], inp["means"], inp["vars_"]
    dy, mask, on = inp.pop("dy"), inp.pop("mask"), inp.pop("on")
    dx, dg, db = res[:3]
    g = dy if on is None else np.where(on, dy, F(0))
    del on, mask, dy
    if mode == 3:
        assert np.array_equal(res[3].view(np.uint32), g.view(np.uint32)), "mode 3: the gated dy is not mask > 0 ? dy : 0"
    del res
    sums = E.grad_sums(g, x, means, vars_, EPS)
    bad, ws = E.sums_violations(db, dg, sums)
    assert bad == 0, "dbeta / dgamma: %d values out of bounds (worst %.3g x 2^-24 sum|terms|)" % (bad, ws)
    record(("bn' sums " + pair, "mode %d" % mode), ws)
    slabs = E.bn_dx_slabs(g, x, gamma, means, vars_, EPS, sums, R.slab_images(N, seed=seed), R.slab_channels(Cn, seed))
    w = R.check_slabs(dx, slabs, x_dt == BF16, "%s %s mode %d dx" % (pair, (Cn, H), mode))
    record(("bn' dx " + pair, "mode %d" % mode), w)
    print("%s: dx worst %.3g, sums worst %.3g (%.1f s)" % (case, w, ws, time.time() - t0))


def _relu_pattern(shape, seed, dt):
    return _round_(np.maximum(pattern(shape, seed), 0), dt)


def maxpool_inputs(dt, N, Cn, H, cheap=False):
    x = _relu_pattern((N, Cn, H, H), 51, dt) if cheap else relu_normal((N, Cn, H, H), 51, dt)
    x[..., 1::4, :] = x[..., 0::4, :]      # rows 4j and 4j + 1 equal: ties inside every window that spans both
    x[..., :, 2::6] = x[..., :, 1::6]      # columns 6j + 1 and 6j + 2 equal: ties across the overlap column of two windows
    shp = (N, Cn, H // 2, H // 2)
    dy = _rnd(dt)(pattern(shp, 52) if cheap else np.random.default_rng(52).standard_normal(shp, dtype=F))
    return dict(x=x, dy=dy)


def maxpool_fwd_call(ops, dt, inp):
    return ops.maxpool_fwd_t(inp["x"], 3, 2, dt)


def maxpool_bwd_call(ops, dt, inp, idx):
    return ops.maxpool_bwd_t(idx, inp["dy"], inp["x"].shape[2], 3, 2, dt)


def maxpool(ops, dt, N, Cn, H, record):
    """the stem's max-pool (maxpool_fwd_3x3s2_kernel / maxpool_bwd_3x3s2_kernel): values, arg-max indices and dx bit for bit against the
    documented rule, on post-ReLU input with planted ties inside windows and across the overlaps of neighbouring windows"""
    inp = maxpool_inputs(dt, N, Cn, H)
    x, dy = inp["x"], inp["dy"]
    y, idx = maxpool_fwd_call(ops, dt, inp)
    ry, ridx = E.maxpool_fwd_ref(x)
    assert np.array_equal(y.view(np.uint32), ry.view(np.uint32)), "max-pool values: %d differ" % np.count_nonzero(y != ry)
    assert np.array_equal(idx, ridx), "max-pool indices: %d differ" % np.count_nonzero(idx != ridx)
    del y, ry, ridx
    assert dy.shape == idx.shape
    dx = maxpool_bwd_call(ops, dt, inp, idx)
    rdx = E.maxpool_bwd_ref(idx, dy, H)
    assert np.array_equal(dx.view(np.uint32), rdx.view(np.uint32)), "max-pool dx: %d differ" % np.count_nonzero(dx != rdx)
    record(("maxpool " + ("bf16" if dt else "f32"), "fwd, bwd"), 0.0)


def avgpool_inputs(dt, N, Cn, H, cheap=False):
    if cheap:
        return dict(x=_relu_pattern((N, Cn, H, H), 61, dt), dy=pattern((N, Cn), 62))
    return dict(x=relu_normal((N, Cn, H, H), 61, dt), dy=np.random.default_rng(62).standard_normal((N, Cn), dtype=F))


def avgpool_call(ops, dt, inp):
    """returns (y, dx)"""
    return ops.avgpool_fwd_t(inp["x"], dt), ops.avgpool_bwd_t(inp["dy"], inp["x"].shape[2], dt)


def avgpool(ops, dt, N, Cn, H, record):
    """the forward (H^2-term sums) against float64; the backward dy / H^2 in fp32, stored: bit for bit"""
    inp = avgpool_inputs(dt, N, Cn, H)
    x, dy = inp["x"], inp["dy"]
    y, dx = avgpool_call(ops, dt, inp)
    ref, A = E.avgpool_ref(x)
    w, bad = R.dist_f32(y, ref, A)
    assert bad == 0, "avgpool forward: %d out of bounds (worst %.3g)" % (bad, w)
    record(("avgpool fwd " + ("bf16 in" if dt else "f32"), ""), w)
    rdx = _rnd(dt)(np.broadcast_to((dy / F(H * H))[:, :, None, None], dx.shape).astype(F))
    assert np.array_equal(dx.view(np.uint32), rdx.view(np.uint32)), "avgpool dx: %d differ" % np.count_nonzero(dx != rdx)


def softmax_ce_inputs(N, Ln):
    return dict(x=E.softmax_rows(N, Ln, 71), labels=synth.labels(72, N, Ln))


def softmax_ce_call(ops, inp):
    """returns (soft-max, ce_deriv of it)"""
    got = ops.softmax(inp["x"])
    return got, ops.ce_deriv(got, inp["labels"])


def softmax_ce(ops, N, Ln, record):
    """N x Ln logits, with rows at |x| ~ 80-110 and rows of many equal maxima: soft-max against float64; ce_deriv = pred - onehot bit for
    bit (float32)"""
    inp = softmax_ce_inputs(N, Ln)
    x, labels = inp["x"], inp["labels"]
    got, d = softmax_ce_call(ops, inp)
    ref, A = E.softmax_ref(x)
    w, bad = R.dist_f32(got, ref, A)
    assert bad == 0, "soft-max: %d out of bounds (worst %.3g)" % (bad, w)
    record(("softmax", ""), w)
    exp = got.copy()
    exp[np.arange(N), labels] -= F(1)
    assert np.array_equal(d.view(np.uint32), exp.view(np.uint32)), "ce_deriv: %d differ" % np.count_nonzero(d != exp)


def nhwc_to_nchw_inputs(N, H):
    return synth.uniform(90, N * H * H * 3, -124.0, 152.0).reshape(N, H, H, 3)


def nhwc_to_nchw(ops, N, H):
    im = nhwc_to_nchw_inputs(N, H)
    got = ops.nhwc_to_nchw(im)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(im.transpose(0, 3, 1, 2)).view(np.uint32))
