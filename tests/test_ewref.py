"""The checker of test_gpu_batch256_ew.py on the CPU (no GPU): float32 executions of batch norm, soft-max and Adam, summed in other
orders than the kernels, pass its bounds; numpy mutants of the mistakes these kernels could make fail them; its case list covers every
batch-norm site forward_pass and backwards_pass produce for ResNet-50."""
import numpy as np
import pytest

import convref as R
import ewref as E

F = np.float32
N, EPS = 8, E.EPS


@pytest.fixture(scope="module", autouse=True)
def _threads():
    R.set_threads(16)


def _x(Cn, H, seed, bf=False):
    """a convolution output with per-channel scales 1e-3 .. 3 (small variances make eps matter) and offsets of up to 2 standard deviations"""
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(3.0), Cn))
    off = rng.uniform(-2, 2, Cn) * scale
    x = (rng.standard_normal((N, Cn, H, H)) * scale[None, :, None, None] + off[None, :, None, None]).astype(F)
    return R.bf16_round32(x) if bf else x


def _params(Cn, seed):
    rng = np.random.default_rng(seed)
    gamma = (1 + 0.3 * rng.standard_normal(Cn)).astype(F)
    beta = (0.3 * rng.standard_normal(Cn)).astype(F)
    beta[::4] = 0                                    # channels where y == 0 exactly at x == mean
    return gamma, beta


# ---------------------------------------------------------------------------------------------------------------------------
# batch-norm statistics: per split (images split, split + ns, ...) a float32 two-pass, splits merged in float32 (Chan)
def _stats_split_f32(x, ns, drop=None):
    Cn = x.shape[1]
    n, mean, m2 = np.zeros(Cn, F), np.zeros(Cn, F), np.zeros(Cn, F)
    for sp in range(ns):
        if sp == drop:
            continue
        xs = x[sp::ns]
        cnt = F(xs.shape[0] * xs.shape[2] * xs.shape[3])
        mu = xs.sum((0, 2, 3), dtype=F) / cnt
        d = xs - mu[None, :, None, None]
        q = (d * d).sum((0, 2, 3), dtype=F)
        tot = n + cnt
        dd = mu - mean
        fr = cnt / tot
        m2 = (m2 + q + dd * dd * n * fr).astype(F)
        mean = (mean + dd * fr).astype(F)
        n = tot
    return mean, (m2 / n).astype(F)


@pytest.mark.parametrize("bf", [False, True])
def test_bn_statistics_valid_pass_dropped_split_fails(bf):
    x = _x(16, 7, 1, bf)
    gm, gv = _stats_split_f32(x, 4)
    assert E.stats_violations(gm, gv, x)[0] == 0
    gm, gv = _stats_split_f32(x, 4, drop=3)
    assert E.stats_violations(gm, gv, x)[0] > 0


# ---------------------------------------------------------------------------------------------------------------------------
# batch-norm apply as the vector kernel runs it: V consecutive elements of the flattened tensor; on 7x7 planes a vector runs into the next
# channel's plane (and from channel C - 1 into channel 0 of the next image) -- the straddle form
def _apply_f32(x, gamma, beta, means, vars_, relu, residual=None, V=1, straddle_bug=False):
    Nn, Cn, H, _ = x.shape
    P = H * H
    e = np.arange(x.size)
    c = (e // P) % Cn
    if straddle_bug:
        c = ((e // V * V) // P) % Cn                  # the spill elements keep the vector's first channel
    sd = np.sqrt(vars_ + F(EPS)).astype(F)
    xf = x.ravel()
    y = (gamma[c] * ((xf - means[c]) / sd[c]) + beta[c]).astype(F)
    if residual is not None:
        y = np.maximum(y + residual.ravel(), F(0))
    elif relu:
        y = np.maximum(y, F(0))
    return y.reshape(x.shape)


@pytest.mark.parametrize("form", ["relu", "none", "add_relu"])
@pytest.mark.parametrize("bf", [False, True])
def test_bn_apply_valid_pass_straddle_mutant_fails(form, bf):
    Cn, H = 16, 7
    x = _x(Cn, H, 2, bf)
    gamma, beta = _params(Cn, 3)
    means, vars_ = (a.astype(F) for a in E.stats_ref(x)[:2])
    res = R.bf16_round32(np.maximum(np.random.default_rng(4).standard_normal(x.shape).astype(F), 0)) if form == "add_relu" else None
    relu = form != "none"
    rnd = R.bf16_round32 if bf else (lambda a: a)
    S, Rc = R.slab_images(N), R.slab_channels(Cn)
    slabs = E.bn_apply_slabs(x, gamma, beta, means, vars_, EPS, relu, res, S, Rc)
    got = rnd(_apply_f32(x, gamma, beta, means, vars_, relu, res, V=8 if bf else 4))
    assert R.violations(got, slabs, bf) == 0
    bad = rnd(_apply_f32(x, gamma, beta, means, vars_, relu, res, V=8 if bf else 4, straddle_bug=True))
    assert R.violations(bad, slabs, bf) > 0


def test_channel_last_copy_layouts():
    y = np.arange(2 * 3 * 4 * 4, dtype=F).reshape(2, 3, 4, 4) + 1
    pl = E.channel_last(y, False)
    assert pl.shape == (2, 6, 6, 3) and pl[1, 2, 3, 1] == y[1, 1, 1, 2] and pl[:, 0].sum() == 0 and pl[:, :, -1].sum() == 0
    pp = E.channel_last(y, True)
    assert pp.shape == (2, 4, 3, 3, 3) and pp[1, 2 * 1 + 0, 1 + 1, 1 + 1, 2] == y[1, 2, 3, 2] and pp[:, :, 0].sum() == 0
    assert np.count_nonzero(pp) == y.size and np.count_nonzero(pl) == y.size


# ---------------------------------------------------------------------------------------------------------------------------
# batch-norm backward in float32: sums per image, images added in reverse; dx from the float32 sums
def _bwd_f32(x, dy, gamma, beta, means, vars_, mode, mask=None, gate_ge=False, no_k1=False, eps_outside=False):
    sd = (np.sqrt(vars_) + F(EPS)).astype(F) if eps_outside else np.sqrt(vars_ + F(EPS)).astype(F)
    c = lambda v: v[None, :, None, None]
    xh = ((x - c(means)) / c(sd)).astype(F)
    if mode == 1:
        y = (c(gamma) * xh + c(beta)).astype(F)
        on = y >= 0 if gate_ge else y > 0
    elif mode == 3:
        on = mask > 0
    else:
        on = np.ones(x.shape, bool)
    g = np.where(on, dy, F(0)).astype(F)
    db, dg = np.zeros(x.shape[1], F), np.zeros(x.shape[1], F)
    for n in reversed(range(x.shape[0])):
        db = (db + g[n].sum((1, 2), dtype=F)).astype(F)
        dg = (dg + (g[n] * xh[n]).sum((1, 2), dtype=F)).astype(F)
    M = F(x.shape[0] * x.shape[2] * x.shape[3])
    k1 = F(0) * db if no_k1 else db / M
    dx = (c(gamma / sd) * (g - c(k1) - xh * c(dg / M))).astype(F)
    return dx, dg, db, g


def _bwd_data(mode, bf):
    Cn, H = 16, 8
    x = _x(Cn, H, 5, bf)
    gamma, beta = _params(Cn, 6)
    mu, var = E.stats_ref(x)[:2]
    means, vars_ = R.bf16_round32(mu.astype(F)), var.astype(F)
    rng = np.random.default_rng(7)
    dy = (rng.standard_normal(x.shape) + rng.uniform(-0.5, 0.5, Cn)[None, :, None, None]).astype(F)
    if bf:
        dy = R.bf16_round32(dy)
    mask = R.bf16_round32(np.maximum(rng.standard_normal(x.shape).astype(F), 0)) if mode == 3 else None
    if mode == 1:                                    # x == mean exactly in the beta == 0 channels: y == 0, the gate is shut
        x[:, ::4, ::3, ::2] = means[::4][None, :, None, None]
    return x, dy, gamma, beta, means, vars_, mask


def _bwd_check(x, dy, gamma, beta, means, vars_, mode, mask, got_dx, got_dg, got_db, bf):
    if mode == 1:
        y, _ = E.bn_gate_y(x, gamma, beta, means, vars_, EPS)
        on = y > 0
    elif mode == 3:
        on = mask > 0
    else:
        on = np.ones(x.shape, bool)
    g = np.where(on, dy, F(0))
    sums = R.bn_grad_sums(g, x, means, vars_, EPS)
    sbad, _ = E.sums_violations(got_db, got_dg, sums)
    slabs = E.bn_dx_slabs(g, x, gamma, means, vars_, EPS, sums, R.slab_images(x.shape[0]), R.slab_channels(x.shape[1]))
    return sbad + R.violations(got_dx, slabs, bf)


@pytest.mark.parametrize("mode", [1, 3, 0])
@pytest.mark.parametrize("bf", [False, True])
def test_bn_backward_valid_pass_mutants_fail(mode, bf):
    data = _bwd_data(mode, bf)
    rnd = R.bf16_round32 if bf else (lambda a: a)
    dx, dg, db, _ = _bwd_f32(*data[:6], mode, data[6])
    assert _bwd_check(*data[:6], mode, data[6], rnd(dx), dg, db, bf) == 0
    for mut in ("no_k1", "eps_outside") + (("gate_ge",) if mode == 1 else ()):
        dx, dg, db, _ = _bwd_f32(*data[:6], mode, data[6], **{mut: True})
        assert _bwd_check(*data[:6], mode, data[6], rnd(dx), dg, db, bf) > 0, mut


# ---------------------------------------------------------------------------------------------------------------------------
def _maxpool_loops(x):
    """the rule by plain loops (a 2 x 2 x 16 x 16 tensor): the restatement itself is checked"""
    Nn, Cn, H, _ = x.shape
    Ho = H // 2
    y = np.zeros((Nn, Cn, Ho, Ho), F); idx = np.zeros((Nn, Cn, Ho, Ho), np.int32)
    dyv = np.arange(1, y.size + 1, dtype=F).reshape(y.shape)
    dx = np.zeros(x.size, F)
    for n in range(Nn):
        for c in range(Cn):
            for oh in range(Ho):
                for ow in range(Ho):
                    mv, mi = -1024.0, -1024
                    for r in (-1, 0, 1):
                        for cc in (-1, 0, 1):
                            ih, iw = 2 * oh + r, 2 * ow + cc
                            if 0 <= ih < H and 0 <= iw < H and x[n, c, ih, iw] > mv:
                                mv, mi = x[n, c, ih, iw], ((n * Cn + c) * H + ih) * H + iw
                    y[n, c, oh, ow], idx[n, c, oh, ow] = mv, mi
                    dx[mi] = dyv[n, c, oh, ow]                 # scan order: the last writer stays
    return y, idx, dyv, dx.reshape(x.shape)


def _pool_input(shape, seed):
    """post-ReLU values (about half exact zeros) with planted ties inside windows and across window overlaps"""
    rng = np.random.default_rng(seed)
    x = R.bf16_round32(np.maximum(rng.standard_normal(shape).astype(F), 0))
    x[..., 1::4, :] = x[..., 0::4, :][..., :x[..., 1::4, :].shape[-2], :]   # equal rows: ties in every window that spans both
    x[..., :, 2::6] = x[..., :, 1::6][..., :x[..., :, 2::6].shape[-1]]      # equal columns across the overlap column 2 ow + 1
    return x


def test_maxpool_restatement_matches_loops_and_mutants_fail():
    x = _pool_input((2, 2, 16, 16), 8)
    y0, i0, dy, dx0 = _maxpool_loops(x)
    y, idx = E.maxpool_fwd_ref(x)
    assert np.array_equal(y, y0) and np.array_equal(idx, i0)
    assert np.array_equal(E.maxpool_bwd_ref(idx, dy, 16), dx0)
    _, il = E.maxpool_fwd_ref(x, last_max=True)
    assert not np.array_equal(il, i0), "ties must decide the index"
    assert not np.array_equal(E.maxpool_bwd_ref(idx, dy, 16, first_writer=True), dx0), "overlaps must decide the writer"


# ---------------------------------------------------------------------------------------------------------------------------
def test_softmax_valid_pass_no_max_subtraction_fails():
    x = E.softmax_rows(16, 1000, 9)
    ref, A = E.softmax_ref(x)
    assert R.dist_f32(E.softmax_f32(x), ref, A)[1] == 0
    assert R.dist_f32(E.softmax_f32(x.astype(np.float64).astype(F)[:, ::-1].copy(), True)[:, ::-1], ref, A)[1] == 0  # another summation order
    assert R.dist_f32(E.softmax_f32(x, subtract_max=False), ref, A)[1] > 0


def test_avgpool_bound_accepts_float32():
    x = R.bf16_round32(np.random.default_rng(10).standard_normal((4, 64, 7, 7)).astype(F))
    ref, A = E.avgpool_ref(x)
    got = x.reshape(4, 64, 49)[..., ::-1].sum(2, dtype=F) / F(49)
    assert R.dist_f32(got, ref, A)[1] == 0
    assert R.dist_f32(x.reshape(4, 64, 49)[..., 1:].sum(2, dtype=F) / F(49), ref, A)[1] > 0   # a missing term


# ---------------------------------------------------------------------------------------------------------------------------
def _adam_state(n, seed):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 0.05).astype(F)
    g = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 2, n))).astype(F)
    m = (rng.standard_normal(n) * 1e-2).astype(F)
    v = (np.abs(rng.standard_normal(n)) * 1e-4).astype(F)
    return p, g, m, v


def _decay(b, t):
    c = F(1)
    for _ in range(t):
        c = F(c * F(b))
    return c


@pytest.mark.parametrize("t", [1, 500])
def test_adam_valid_pass_bias_correction_mutant_fails(t):
    p, g, m, v = _adam_state(100000, 11)
    g[[5, 77, -1]] = [np.nan, np.inf, -np.inf]
    hp = dict(lr=1e-3, wd=5e-4, b1=0.9, b2=0.999, cb1=_decay(0.9, t), cb2=_decay(0.999, t), eps=1e-7)
    got = E.adam_f32(p, g, m, v, **hp)
    refs = E.adam_ref(p, g, m, v, **hp)
    for a, (ref, A) in zip(got, refs):
        assert R.dist_f32(a, ref, A)[1] == 0
    assert np.array_equal(got[1][[5, 77, -1]], m[[5, 77, -1]]) and np.array_equal(got[2][[5, 77, -1]], v[[5, 77, -1]])
    if t > 1:
        refb = E.adam_ref(p, g, m, v, bias_b=True, **hp)[0]
        assert R.dist_f32(got[0], *refb)[1] > 0


def test_nan_is_out_of_bounds():
    ref, A = np.ones(4), np.ones(4)
    got = np.array([1, np.nan, 1, 1], F)
    assert R.dist_f32(got, ref, A)[1] == 1 and R.dist_bf16(got, ref, A)[1] == 1
    assert R.dist_f32(got, ref, A)[0] == float("inf") and R.dist_bf16(got, ref, A)[0] == float("inf")


def test_arena_is_the_trainers():
    import ctypes as C
    import synth
    from resnet_amd import binding as B
    L = B.load()
    dims = synth.R50_DIMS
    n = E.arena_floats(dims)
    assert n > 2 ** 24
    flags = (C.c_int * dims["n_conv_blocks"])(*dims["is_block_spatial_reduction"])
    d = L.init_dimensions(dims["input"], dims["init_kernel_dim"], dims["init_conv_filters"], dims["init_conv_stride"],
                          dims["init_maxpool_dim"], dims["init_maxpool_stride"], dims["n_conv_blocks"], flags, dims["final_depth"], dims["output"])
    assert L.mi_debug_arena_floats(d) == n


# ---------------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_every_trainer_bn_site():
    """every (storage pair, C, H, form / mode) of ResNet-50's forward_pass and backwards_pass at N = 256 is a case of
    test_gpu_batch256_ew.py, or (BN' with the reduction done by the dgrad) a dgrad case of test_gpu_batch256.py"""
    from resnet_amd import binding as B
    L = B.load()
    sites = E.trainer_bn_sites(L)
    have = {(pr, Cn, H, "fwd", f) for pr, Cn, H, forms in E.bn_fwd_cases() for f in forms}
    have |= {(pr, Cn, H, "bwd", m) for pr, Cn, H, m in E.bn_bwd_cases()}
    have |= {(dt, Cn, H, "bwd", "parts") for dt, Cn, H, K, k, s, where in R.dgrad_bn_cases(L)}
    missing = sorted(sites - have, key=str)
    assert not missing, missing
    kinds = {(k[3], k[4]) for k in sites}
    for want in (("fwd", "cl plane"), ("fwd", "cl par"), ("fwd", "cl par add_relu"), ("bwd", 0), ("bwd", 1), ("bwd", 3), ("bwd", "parts")):
        assert want in kinds, want
    print("\n%d trainer sites, %d forward and %d backward cases" % (len(sites), len(E.bn_fwd_cases()), len(E.bn_bwd_cases())))


def test_bn_lists_from_dims_are_the_batch256_lists():
    """bn_shapes / trainer_bn_fwd_cases / trainer_bn_bwd_cases of ResNet-50 are BN_SHAPES and the case lists of test_gpu_batch256_ew.py"""
    import synth
    assert E.bn_shapes(synth.R50_DIMS) == E.BN_SHAPES
    assert E.trainer_bn_fwd_cases(synth.R50_DIMS) == E.bn_fwd_cases()
    assert E.trainer_bn_bwd_cases(synth.R50_DIMS) == E.bn_bwd_cases()


@pytest.mark.parametrize("net,n", [("r50", 33), ("c1s", 4), ("c4i", 4), ("r50", 8)])
def test_ragged_lists_cover_every_trainer_bn_site(net, n):
    """every batch-norm site of the net's trainer at batch n is a case of test_gpu_ragged.py: a forward form or backward mode of the BN
    lists built from its dims, or (BN' with the reduction done by the dgrad) one of its dgrad + BN' cases"""
    from resnet_amd import binding as B
    L = B.load()
    d = R.nets()[net]
    sites = E.trainer_bn_sites(L, d, n)
    have = {(pr, Cn, H, "fwd", f) for pr, Cn, H, forms in E.trainer_bn_fwd_cases(d) for f in forms}
    have |= {(pr, Cn, H, "bwd", m) for pr, Cn, H, m in E.trainer_bn_bwd_cases(d)}
    have |= {(dt, Cn, H, "bwd", "parts") for dt, Cn, H, K, k, s, where in R.trainer_dgrad_bn_cases(L, d, n)}
    missing = sorted(sites - have, key=str)
    assert not missing, missing
    kinds = {(k[3], k[4]) for k in sites}
    for want in (("fwd", "cl plane"), ("fwd", "cl par"), ("fwd", "cl par add_relu"), ("bwd", 0), ("bwd", 1), ("bwd", 3), ("bwd", "parts")):
        assert want in kinds, want
