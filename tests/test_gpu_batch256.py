"""Every convolution route of the reference ResNet-50 at the benchmark's batch (256), element by element against a float64 reference.

The kernel plans depend on N (tile heights, sliced tail rounds, split weight gradients and their grouped reduce): the operator tests at
N <= 16 never reach the plans the benchmark runs.  The case list is convref.batch256_cases: every (layer shape, route) pair plan_layers
gives the network in fp32 and in bf16 storage with default switches, plus the 1x1 forward on a channel-last input.  Each case is checked
per element on the slabs of convref (every channel of a few images, every image of a few channels per 64-channel block), to
64 * 2^-24 * A (A = the same sum over |terms|); bf16 outputs must lie between the RNE roundings of ref -/+ that bound.  The FC GEMM in
its three forms is checked in full.
"""
import os
import time

import numpy as np
import pytest

import convref as R
import ewref as E

pytestmark = pytest.mark.gpu

N = R.N256
WORST = {}  # (dtype, route, op) -> worst distance, printed at the end of the module (bf16: where the bound pins the rounding)


def _cases():
    from resnet_amd import binding as B
    return R.batch256_cases(B.load())


def _record(key, worst):
    WORST[key] = max(WORST.get(key, 0.0), worst)


try:
    from resnet_amd import binding as _B
    _B.load()
except RuntimeError:  # library not built: collection must still work; the tests then fail in the ops fixture
    CASES = []
else:
    CASES = _cases()  # an error in building the case list fails collection loudly
IDS = ["%s_%s_%s_C%d_H%d_K%d_k%d_s%d" % c[:8] for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def _threads():
    R.set_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    yield
    print("\nworst distance per route at N = %d (fp32 and reductions: x 2^-24 A, bf16: bf16 ulps)" % N)
    for key in sorted(WORST):
        print("  %-4s %-7s %-9s %.3g" % (key + (WORST[key],)))


def _normal(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * np.float32(scale))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_conv_route_at_batch_256(ops, case):
    dt, route, op, Cn, H, K, k, s, where = case
    bf = dt == "bf16"
    Ho = H // s
    L = ops.L
    plan = R.conv_plan(L, 1 if bf else 0, route, op, N, Cn, H, K, k, s)
    assert plan is not None or (not bf and route == "default"), "%s refuses %s" % (route, case)
    rnd = R.bf16_round32 if bf else (lambda a: a)
    seed = hash((Cn, H, K, k, s)) % 1000
    w = rnd(_normal((K, Cn, k, k), seed + 1, (2.0 / (k * k * (Cn + K))) ** 0.5))
    t0 = time.time()
    if op == "fwd":
        x = rnd(_normal((N, Cn, H, H), seed + 2))
        if route == "default":
            got = ops.conv_fwd_bf16(x, w, s) if bf else ops.conv_fwd(x, w, s)
        elif route == "cl":
            got = ops.conv_fwd_bf16_cl(x, w, s)
        else:
            got = ops.conv1x1_fwd_bf16_cl(x, w)
        Pc = (Ho * Ho + 7) // 8 * 8 if bf and route == "default" else Ho * Ho
        S = R.slab_images(N, plan, K, Pc, seed)
        slabs = R.fwd_slabs(x, w, s, S, R.slab_channels(K, seed))
    elif op == "dgrad":
        dy = rnd(_normal((N, K, Ho, Ho), seed + 3))
        addend = rnd(_normal((N, Cn, H, H), seed + 4)) if "red" in where else None
        if route == "default":
            got = ops.conv_dgrad_bf16(w, dy, H, s, dx_init=addend) if bf else ops.conv_dgrad(w, dy, H, s, dx_init=addend)
        else:
            got = ops.conv_dgrad_bf16_cl(w, dy, H, dx_init=addend, stride=s)
        Pc = (H * H + 7) // 8 * 8 if bf and route == "default" else H * H
        S = R.slab_images(N, plan, Cn, Pc, seed)
        slabs = R.dgrad_slabs(w, dy, H, s, S, R.slab_channels(Cn, seed), addend)
    else:
        x = rnd(_normal((N, Cn, H, H), seed + 2))
        dy = rnd(_normal((N, K, Ho, Ho), seed + 3))
        if route == "default" or route == "pw":
            got = ops.conv_wgrad_bf16(x, dy, k, s) if bf else ops.conv_wgrad(x, dy, k, s)
        elif route == "cl":
            got = ops.conv_wgrad_bf16_cl(x, dy, s)
        else:
            got = ops.conv_wgrad_bf16_cl2(x, dy, s)
        slabs = R.wgrad_slabs(x, dy, k, s, R.slab_channels(K, seed), R.slab_channels(Cn, seed + 1))
    # the weight gradient is fp32 on every route; fwd / dgrad outputs are stored as bf16 on the bf16 routes
    out_bf = bf and op != "wgrad"
    t1 = time.time()
    worst = R.check_slabs(got, slabs, out_bf, "%s %s %s %s" % (dt, route, op, (Cn, H, K, k, s)))
    _record((dt, route, op), worst)
    print("%s plan %s: worst %.3g %s (kernel, transfers and reference %.1f s, check %.1f s)"
          % (case, plan, worst, "bf16 ulp" if out_bf else "x 2^-24 A", t1 - t0, time.time() - t1))


@pytest.mark.parametrize("form", ["nn", "lt", "rt"])
def test_fc_gemm_at_batch_256(ops, form):
    """the FC layer's three products at 256 x 2048 x 1000: logits = X W, dW = X^T dY, dX = dY W^T (full float64 reference)"""
    X = np.maximum(_normal((N, 2048), 31), 0)  # pooled ReLU features
    W = _normal((2048, 1000), 32, 0.01)
    dY = _normal((N, 1000), 33)
    if form == "nn":
        a, b = X, W
        got = ops.matmul(a, b, "nn")
        ref, A = a.astype(np.float64) @ b, np.abs(a).astype(np.float64) @ np.abs(b)
    elif form == "lt":
        a, b = X, dY
        got = ops.matmul(a, b, "lt")
        ref, A = a.T.astype(np.float64) @ b, np.abs(a.T).astype(np.float64) @ np.abs(b)
    else:
        a, b = dY, W
        got = ops.matmul(a, b, "rt")
        ref, A = a.astype(np.float64) @ b.T, np.abs(a).astype(np.float64) @ np.abs(b.T)
    worst, bad = R.dist_f32(got, ref, A)
    assert bad == 0, "FC %s: %d elements out of bounds (worst %.3g x 2^-24 A)" % (form, bad, worst)
    WORST[("f32", "fc", form)] = worst


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("op", ["fwd", "wgrad"])
def test_stem_at_batch_256(ops, dt, op):
    """the 7x7 stride-2 stem on its matrix-core kernels (exact fp32, or bf16 operands with fp32 accumulation; fp32 tensors either way):
    the forward on the slabs, the weight gradient against the full float64 reduction over every image"""
    Cn, H, K, k, s = R.STEM
    bf = dt == "bf16"
    rnd = R.bf16_round32 if bf else (lambda a: a)
    x = rnd(_normal((N, Cn, H, H), 41, 60.0))                       # images of the scale the batch source gives (about +-124)
    w = rnd(_normal((K, Cn, k, k), 42, (2.0 / (k * k * (Cn + K))) ** 0.5))
    if op == "fwd":
        got = ops.stem_fwd_bf16(x, w, exact=not bf)
        slabs = R.fwd_slabs(x, w, s, R.slab_images(N, seed=7), R.slab_channels(K, 7))
    else:
        dy = rnd(_normal((N, K, H // s, H // s), 43))
        got = ops.stem_wgrad_bf16(x, w, dy, exact=not bf)
        slabs = R.wgrad_slabs(x, dy, k, s, list(range(K)), [])     # every row: the whole weight gradient
    worst = R.check_slabs(got, slabs, False, "stem %s %s" % (dt, op))
    _record((dt, "stem", op), worst)
    print("stem %s %s: worst %.3g x 2^-24 A" % (dt, op, worst))


def _bn_params(Cn, seed):
    gamma = (1 + 0.2 * _normal((Cn,), seed)).astype(np.float32)
    beta = (0.3 * _normal((Cn,), seed + 1)).astype(np.float32)
    return gamma, beta


CONV_BN = R.conv_bn_cases()


@pytest.mark.parametrize("case", CONV_BN, ids=["%s_C%d_H%d_K%d_k%d_s%d" % c[:6] for c in CONV_BN])
def test_conv_bn_fwd_at_batch_256(ops, case):
    """mi_op_conv_bn_fwd_t as forward_pass pairs a convolution with its BN: the BN statistics come from the convolution's epilogue
    (including the partial rows the sliced tail tiles write).  The convolution output is checked on the slabs; the means and variances
    of the channels in R against the float64 statistics of the exact convolution over all images, to C_FACTOR 2^-24 times the sum of
    |terms| plus what the convolution's own bound carries in (contract: statistics of the fp32 accumulators, before any rounding)"""
    dt, Cn, H, K, k, s, where = case
    bf = dt == "bf16"
    rnd = R.bf16_round32 if bf else (lambda a: a)
    seed = hash((Cn, H, K, k, s)) % 1000 + 500
    x = rnd(_normal((N, Cn, H, H), seed + 2))
    w = rnd(_normal((K, Cn, k, k), seed + 1, (2.0 / (k * k * (Cn + K))) ** 0.5))
    gamma, beta = _bn_params(K, seed + 3)
    conv, gm, gv, y, fused = ops.conv_bn_fwd_t(x, w, gamma, beta, s, 1e-7, 1, 1 if bf else 0)
    assert fused, "every layer tiles: the statistics must come from the convolution's epilogue"
    plan = R.conv_plan(ops.L, 1 if bf else 0, "default", "fwd", N, Cn, H, K, k, s)
    Ho = H // s
    Pc = (Ho * Ho + 7) // 8 * 8 if bf else Ho * Ho
    Rk, S = R.slab_channels(K, seed), R.slab_images(N, plan, K, Pc, seed)
    slabs = R.fwd_slabs(x, w, s, S, Rk)
    worst = R.check_slabs(conv, slabs, bf, "conv_bn %s %s" % (dt, (Cn, H, K, k, s)))
    _record((dt, "default", "fwd+bn"), worst)
    mu, var, bm, bv = R.bn_stats_ref(slabs[1].ref, slabs[1].A)
    em, ev = np.abs(gm[Rk] - mu), np.abs(gv[Rk] - var)
    assert np.all(em <= bm), "means: %d of %d channels out of bounds, worst %.3g of the bound" % (np.sum(em > bm), len(Rk), np.max(em / bm))
    assert np.all(ev <= bv), "vars: %d of %d channels out of bounds, worst %.3g of the bound" % (np.sum(ev > bv), len(Rk), np.max(ev / bv))
    ws = float(max(np.max(em / bm), np.max(ev / bv))) * R.C_FACTOR
    _record((dt, "bn stats", "fwd"), ws)
    # the BN + ReLU output: the float64 apply of the stored convolution output with the statistics the epilogue produced (ewref)
    wy = R.check_slabs(y, E.bn_apply_slabs(conv, gamma, beta, gm, gv, 1e-7, True, None, S, Rk), bf,
                       "conv_bn y %s %s" % (dt, (Cn, H, K, k, s)))
    _record((dt, "bn apply", "fwd+bn"), wy)
    print("%s plan %s: conv worst %.3g %s, statistics worst %.3g x 2^-24 (bound scale), y worst %.3g"
          % (case, plan, worst, "bf16 ulp" if bf else "x 2^-24 A", ws, wy))


DGRAD_BN = R.dgrad_bn_cases()


@pytest.mark.parametrize("case", DGRAD_BN, ids=["%s_C%d_H%d_K%d_k%d_s%d" % c[:6] for c in DGRAD_BN])
def test_dgrad_bn_bwd_at_fused_sites(ops, case):
    """mi_op_conv_dgrad_bn_bwd_{f32,bf16} at the trainer's BN'-fusion sites: the gated dgrad (mask > 0 ? dgrad (+ addend) : 0) on the
    slabs against the convolution reference; dbeta and dgamma against float64 sums of the product's own gated output as it is stored
    (the kernels' contract: kernels_igemm_bf16.hip sums the rounded gradient), to C_FACTOR 2^-24 sum |terms|"""
    dt, Cn, H, K, k, s, where = case
    bf = dt == "bf16"
    rnd = R.bf16_round32 if bf else (lambda a: a)
    seed = hash((Cn, H, K, k, s)) % 1000 + 700
    eps = 1e-7
    w = rnd(_normal((K, Cn, k, k), seed + 1, (2.0 / (k * k * (Cn + K))) ** 0.5))
    dy = rnd(_normal((N, K, H // s, H // s), seed + 2))
    addend = rnd(_normal((N, Cn, H, H), seed + 3)) if "red" in where else None
    bn_x = rnd(_normal((N, Cn, H, H), seed + 4, 1.5) + np.float32(0.3))    # the convolution output the batch norm normalised
    gamma, beta = _bn_params(Cn, seed + 5)
    means = bn_x.mean((0, 2, 3), dtype=np.float64).astype(np.float32)
    vars_ = bn_x.var((0, 2, 3), dtype=np.float64).astype(np.float32)
    sd = np.sqrt(vars_ + np.float32(eps))
    mask = rnd(np.maximum(gamma[None, :, None, None] * ((bn_x - means[None, :, None, None]) / sd[None, :, None, None]) + beta[None, :, None, None], 0))
    fn = ops.conv_dgrad_bn_bwd_bf16 if bf else ops.conv_dgrad_bn_bwd_f32
    gated, bdx, dg, db, fused = fn(w, dy, H, s, bn_x, mask, gamma, beta, means, vars_, eps, addend=addend)
    assert fused == (not bf or (H * H) % 4 == 0), "which launches fuse the BN' reduction"
    plan = R.conv_plan(ops.L, 1 if bf else 0, "default", "dgrad", N, Cn, H, K, k, s)
    Pc = (H * H + 7) // 8 * 8 if bf else H * H
    S, Rc = R.slab_images(N, plan, Cn, Pc, seed), R.slab_channels(Cn, seed)
    slabs = R.gate_slabs(R.dgrad_slabs(w, dy, H, s, S, Rc, addend), mask)
    worst = R.check_slabs(gated, slabs, bf, "gated dgrad %s %s" % (dt, (Cn, H, K, k, s)))
    _record((dt, "default", "dgrad+bn'"), worst)
    rdb, rdg, adb, adg = R.bn_grad_sums(gated, bn_x, means, vars_, eps)
    eb, eg = np.abs(db - rdb), np.abs(dg - rdg)
    bb, bg = R.C_FACTOR * R.U24 * adb, R.C_FACTOR * R.U24 * adg
    assert np.all((eb <= bb) | ((adb == 0) & (db == 0))), "dbeta: %d of %d channels out of bounds" % (np.sum(eb > bb), Cn)
    assert np.all((eg <= bg) | ((adg == 0) & (dg == 0))), "dgamma: %d of %d channels out of bounds" % (np.sum(eg > bg), Cn)
    ws = float(max(np.max(eb / np.maximum(adb * R.U24, 1e-300)), np.max(eg / np.maximum(adg * R.U24, 1e-300))))
    _record((dt, "bn' sums", "bwd"), ws)
    # BN' dx (mid_bn_bwd_parts_t where fused: the merged partials, then bn_bwd_apply_kernel) against the float64 formula from the sums
    wx = R.check_slabs(bdx, E.bn_dx_slabs(gated, bn_x, gamma, means, vars_, eps, (rdb, rdg, adb, adg), S, Rc), bf, "BN' dx %s %s" % (dt, (Cn, H, K, k, s)))
    _record((dt, "bn' dx", "bwd"), wx)
    print("%s plan %s fused %s: gated worst %.3g %s, dbeta / dgamma worst %.3g x 2^-24 sum|terms|, dx worst %.3g"
          % (case, plan, fused, worst, "bf16 ulp" if bf else "x 2^-24 A", ws, wx))
