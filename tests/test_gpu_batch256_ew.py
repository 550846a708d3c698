"""The element-wise half of the training step at the benchmark's batch (256), element by element against float64 references
(tests/ewref.py, bounds of tests/convref.py): batch norm forward (statistics; apply with ReLU, without, with the shortcut add, and the bf16
dual write of a channel-last copy) and backward (modes 1, 3, 0) at every (C, H) of ResNet-50 in every storage pair the trainer uses,
max-pool 3x3 / 2 over the stem output, average pool, soft-max and the cross-entropy derivative, Adam over an arena of ResNet-50's size,
and the NHWC -> NCHW conversion of the batch.

At N = 256 the kernels run the plans the small-batch tests never reach: 32 statistics splits at C = 64 (1 at C = 2048), the widest vectors,
and on 7x7 planes the straddle form, where a vector that runs into the next channel's plane (from C - 1 into channel 0 of the next image)
takes that channel's scalars.  Per-element checks run on convref's slabs (every channel of a few images, every image of the first, last and
6 seeded channels of every 64-channel block); max-pool, the channel-last copies, the pool gradients, ce_deriv and the conversion are
compared bit for bit over whole tensors.
"""
import os
import resource
import time

import numpy as np
import pytest

import convref as R
import ewref as E
import synth

pytestmark = pytest.mark.gpu

N = R.N256
EPS = E.EPS
F = np.float32
F32, BF16 = 0, 1
PAIRS = {"f32": (F32, F32), "bf16": (BF16, BF16), "f32>bf16": (F32, BF16)}
WORST = {}  # (kernel, form) -> worst distance: 2^-24 A (fp32 outputs, reductions) or bf16 ulps (bf16 outputs); printed at the end


def _record(key, worst):
    WORST[key] = max(WORST.get(key, 0.0), worst)


@pytest.fixture(scope="module", autouse=True)
def _threads():
    R.set_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
    t0 = time.time()
    yield
    print("\nworst distance per kernel and form at N = %d (x 2^-24 A, or bf16 ulps where the output is bf16); module %.0f s"
          % (N, time.time() - t0))
    for key in sorted(WORST):
        print("  %-34s %-22s %.3g" % (key + (WORST[key],)))


@pytest.fixture(autouse=True)
def _host_peak(request):
    """the process's peak host memory after each test (the module is held to about 10 GB)"""
    yield
    print(" [peak host RSS %.2f GB]" % (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20))


def _rnd(dt):
    return R.bf16_round32 if dt == BF16 else (lambda a: a)


def _round_(a, dt):
    """round a to bf16 in place, a few images at a time (host memory)"""
    if dt == BF16:
        for i in range(0, a.shape[0], 16):
            a[i:i + 16] = R.bf16_round32(a[i:i + 16])
    return a


def _conv_out(Cn, H, seed, dt):
    """a convolution output: per-channel scales 1e-3 .. 3 (small variances make eps matter) and offsets of up to 2 standard deviations"""
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(np.log(1e-3), np.log(3.0), Cn)).astype(F)
    off = (rng.uniform(-2, 2, Cn) * scale).astype(F)
    x = rng.standard_normal((N, Cn, H, H), dtype=F)
    x *= scale[None, :, None, None]
    x += off[None, :, None, None]
    return _round_(x, dt)


def _bn_params(Cn, seed):
    rng = np.random.default_rng(seed)
    gamma = (1 + 0.3 * np.clip(rng.standard_normal(Cn), -2.5, 2.5)).astype(F)
    beta = (0.3 * rng.standard_normal(Cn)).astype(F)
    beta[::4] = 0
    return gamma, beta


def _relu_normal(shape, seed, dt):
    x = np.random.default_rng(seed).standard_normal(shape, dtype=F)
    np.maximum(x, 0, out=x)
    return _round_(x, dt)


def _check(got, slabs, bf, key, what):
    w = R.check_slabs(got, slabs, bf, what)
    _record(key, w)
    return w


# ---------------------------------------------------------------------------------------------------------------------------
FWD = E.bn_fwd_cases()


@pytest.mark.parametrize("case", FWD, ids=["%s_C%d_H%d" % c[:3] for c in FWD])
def test_bn_fwd_at_batch_256(ops, case):
    """statistics (bn_stats -> bn_finalize) per channel against float64 over all N * P samples; every apply form of this shape against the
    float64 apply with the kernel's statistics; RECOMPUTE_BN's apply from given statistics; the channel-last copies bit for bit"""
    pair, Cn, H, forms = case
    x_dt, a_dt = PAIRS[pair]
    seed = Cn * 7 + H + 11 * x_dt + 13 * a_dt
    x = _conv_out(Cn, H, seed, x_dt)
    gamma, beta = _bn_params(Cn, seed + 1)
    S, Rc = R.slab_images(N, seed=seed), R.slab_channels(Cn, seed)
    abf = a_dt == BF16
    t0 = time.time()
    gm = gv = None
    for form in forms:
        res = _relu_normal(x.shape, seed + 2, a_dt) if "add_relu" in form else None
        relu = form != "none"
        if form.startswith("cl"):
            m, v, y, ycl = ops.bn_fwd_cl_bf16(x, gamma, beta, EPS, residual=res, par="par" in form)
            exp = E.channel_last(y, "par" in form)
            assert ycl.shape == exp.shape
            assert np.array_equal(ycl.view(np.uint32), exp.view(np.uint32)), \
                "%s: the channel-last copy differs from the NCHW output (or a halo is not zero) at %d elements" % (form, np.count_nonzero(ycl != exp))
            del ycl, exp
        else:
            m, v, y = ops.bn_fwd_t(x, gamma, beta, EPS, relu, x_dt, a_dt, residual=res)
        if gm is None:
            gm, gv = m, v
            bad, ws = E.stats_violations(gm[Rc], gv[Rc], x[:, Rc])
            assert bad == 0, "%s statistics: %d values out of bounds (worst %.3g x 2^-24)" % (pair, bad, ws)
            _record(("bn stats " + pair, "fwd"), ws)
        else:
            assert np.array_equal(m, gm) and np.array_equal(v, gv), "%s: the statistics of one tensor differ between launches" % form
        slabs = E.bn_apply_slabs(x, gamma, beta, gm, gv, EPS, relu, res, S, Rc)
        _check(y, slabs, abf, ("bn apply " + pair, form), "%s %s %s" % (pair, (Cn, H), form))
        if form == "relu":  # RECOMPUTE_BN: the same activation from the stored statistics
            y2 = ops.bn_apply_t(x, gamma, beta, gm, gv, EPS, 1, x_dt, a_dt)
            assert np.array_equal(y2.view(np.uint32), y.view(np.uint32)), "RECOMPUTE_BN's apply differs from the forward's"
            del y2
        del y, res
    print("%s: %s %.1f s" % (case, forms, time.time() - t0))


# ---------------------------------------------------------------------------------------------------------------------------
BWD = E.bn_bwd_cases()


def _nudge(x, gamma, beta, means, vars_, x_dt, exact0):
    """mode 1: move x away from the gate's edge wherever |y| lies within twice its bound of 0 (the elements planted at x == mean in beta == 0
    channels stay: y == 0 exactly there, in any arithmetic); returns the gate y > 0"""
    n = E.STEP
    on = np.empty(x.shape, bool)
    moved = 0
    for i in range(0, N, n):
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


@pytest.mark.parametrize("case", BWD, ids=["%s_C%d_H%d_mode%d" % c for c in BWD])
def test_bn_bwd_at_batch_256(ops, case):
    """mi_op_bn_bwd_t: dbeta, dgamma to C_FACTOR 2^-24 sum|terms| against float64 sums of the gated gradient; dx against the float64
    formula from those sums; mode 3's gated dy bit for bit (mask > 0 ? dy : 0).  The statistics are given, as the trainer gives the stored
    ones; means are bf16 numbers so that x == mean can be planted in either storage type"""
    pair, Cn, H, mode = case
    x_dt, a_dt = PAIRS[pair]
    seed = Cn * 5 + H + 17 * mode + 11 * x_dt + 13 * a_dt + 3000
    x = _conv_out(Cn, H, seed, x_dt)
    gamma, beta = _bn_params(Cn, seed + 1)
    mu, var = E.stats_ref(x)[:2]
    means, vars_ = R.bf16_round32(mu.astype(F)), var.astype(F)
    rng = np.random.default_rng(seed + 2)
    dy = rng.standard_normal(x.shape, dtype=F)
    dy += rng.uniform(-0.5, 0.5, Cn).astype(F)[None, :, None, None]    # channel means of dy: k1 is not negligible
    _round_(dy, a_dt)
    mask = None
    t0 = time.time()
    if mode == 1:
        exact0 = np.zeros(x.shape, bool)
        exact0[:, ::4, ::5, ::3] = True                                   # beta == 0 in every 4th channel
        x[exact0] = np.broadcast_to(means[None, :, None, None], x.shape)[exact0]
        on, moved = _nudge(x, gamma, beta, means, vars_, x_dt, exact0)
        assert not np.any(on & exact0)
        del exact0
    elif mode == 3:
        mask = _relu_normal(x.shape, seed + 3, a_dt)
        on = mask > 0
    else:
        on = None
    res = ops.bn_bwd_t(x, gamma, beta, means, vars_, dy, EPS, mode, x_dt, a_dt, mask_src=mask)
    dx, dg, db = res[:3]
    g = dy if on is None else np.where(on, dy, F(0))
    del on, mask, dy
    if mode == 3:
        assert np.array_equal(res[3].view(np.uint32), g.view(np.uint32)), "mode 3: the gated dy is not mask > 0 ? dy : 0"
    del res
    sums = E.grad_sums(g, x, means, vars_, EPS)
    bad, ws = E.sums_violations(db, dg, sums)
    assert bad == 0, "dbeta / dgamma: %d values out of bounds (worst %.3g x 2^-24 sum|terms|)" % (bad, ws)
    _record(("bn' sums " + pair, "mode %d" % mode), ws)
    slabs = E.bn_dx_slabs(g, x, gamma, means, vars_, EPS, sums, R.slab_images(N, seed=seed), R.slab_channels(Cn, seed))
    w = _check(dx, slabs, x_dt == BF16, ("bn' dx " + pair, "mode %d" % mode), "%s %s mode %d dx" % (pair, (Cn, H), mode))
    print("%s: dx worst %.3g, sums worst %.3g (%.1f s)" % (case, w, ws, time.time() - t0))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_maxpool_3x3s2_at_batch_256(ops, dt):
    """the stem's max-pool (256 x 64 x 112^2, maxpool_fwd_3x3s2_kernel / maxpool_bwd_3x3s2_kernel): values, arg-max indices and dx bit for
    bit against the documented rule, on post-ReLU input with planted ties inside windows and across the overlaps of neighbouring windows"""
    Cn, H = 64, 112
    x = _relu_normal((N, Cn, H, H), 51, dt)
    x[..., 1::4, :] = x[..., 0::4, :]      # rows 4j and 4j + 1 equal: ties inside every window that spans both
    x[..., :, 2::6] = x[..., :, 1::6]      # columns 6j + 1 and 6j + 2 equal: ties across the overlap column of two windows
    y, idx = ops.maxpool_fwd_t(x, 3, 2, dt)
    ry, ridx = E.maxpool_fwd_ref(x)
    assert np.array_equal(y.view(np.uint32), ry.view(np.uint32)), "max-pool values: %d differ" % np.count_nonzero(y != ry)
    assert np.array_equal(idx, ridx), "max-pool indices: %d differ" % np.count_nonzero(idx != ridx)
    del y, ry, ridx
    dy = _rnd(dt)(np.random.default_rng(52).standard_normal(idx.shape, dtype=F))
    dx = ops.maxpool_bwd_t(idx, dy, H, 3, 2, dt)
    rdx = E.maxpool_bwd_ref(idx, dy, H)
    assert np.array_equal(dx.view(np.uint32), rdx.view(np.uint32)), "max-pool dx: %d differ" % np.count_nonzero(dx != rdx)
    _record(("maxpool " + ("bf16" if dt else "f32"), "fwd, bwd"), 0.0)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_avgpool_at_batch_256(ops, dt):
    """256 x 2048 x 7^2: the forward (49-term sums) against float64; the backward dy / 49 in fp32, stored: bit for bit"""
    Cn, H = 2048, 7
    x = _relu_normal((N, Cn, H, H), 61, dt)
    y = ops.avgpool_fwd_t(x, dt)
    ref, A = E.avgpool_ref(x)
    w, bad = R.dist_f32(y, ref, A)
    assert bad == 0, "avgpool forward: %d out of bounds (worst %.3g)" % (bad, w)
    _record(("avgpool fwd " + ("bf16 in" if dt else "f32"), ""), w)
    dy = np.random.default_rng(62).standard_normal((N, Cn), dtype=F)
    dx = ops.avgpool_bwd_t(dy, H, dt)
    rdx = _rnd(dt)(np.broadcast_to((dy / F(H * H))[:, :, None, None], dx.shape).astype(F))
    assert np.array_equal(dx.view(np.uint32), rdx.view(np.uint32)), "avgpool dx: %d differ" % np.count_nonzero(dx != rdx)


def test_softmax_and_ce_deriv_at_batch_256(ops):
    """256 x 1000 logits, with rows at |x| ~ 80-110 and rows of many equal maxima: soft-max against float64; ce_deriv = pred - onehot bit
    for bit (float32)"""
    L = 1000
    x = E.softmax_rows(N, L, 71)
    got = ops.softmax(x)
    ref, A = E.softmax_ref(x)
    w, bad = R.dist_f32(got, ref, A)
    assert bad == 0, "soft-max: %d out of bounds (worst %.3g)" % (bad, w)
    _record(("softmax", ""), w)
    labels = synth.labels(72, N, L)
    d = ops.ce_deriv(got, labels)
    exp = got.copy()
    exp[np.arange(N), labels] -= F(1)
    assert np.array_equal(d.view(np.uint32), exp.view(np.uint32)), "ce_deriv: %d differ" % np.count_nonzero(d != exp)


def _decay(b, t):
    c = F(1)
    for _ in range(t):
        c = F(c * F(b))       # the trainer's float32 product (cur_mean_decay *= base_mean_decay)
    return c


@pytest.mark.parametrize("t,planted", [(1, False), (500, True)], ids=["t1", "t500_nan_inf"])
def test_adam_at_batch_256_arena(ops, t, planted):
    """Adam over an arena of ResNet-50's size (every tensor padded to 64 floats: > 2^24 elements) against the float64 formula from the
    same float32 inputs.  Planted: NaN / +-Inf gradients (the last element among them) keep m and v, and p is then formed from the kept
    moments (the reference's updateParams); an update that overflows keeps p; either sets the flag"""
    n = E.arena_floats(synth.R50_DIMS)
    rng = np.random.default_rng(80 + t)
    p = rng.standard_normal(n, dtype=F) * F(0.05)
    g = rng.standard_normal(n, dtype=F) * np.exp(rng.uniform(-8, 2, n)).astype(F)
    m = rng.standard_normal(n, dtype=F) * F(1e-2)
    v = np.abs(rng.standard_normal(n, dtype=F)) * F(1e-4)
    hp = dict(lr=1e-3, wd=5e-4, b1=0.9, b2=0.999, cb1=_decay(0.9, t), cb2=_decay(0.999, t), eps=1e-7)
    bad_g = np.array([0, 12345, 2 ** 24 + 7, n - 2, n - 1]) if planted else np.array([], int)
    ovf = np.array([99, n - 3]) if planted else np.array([], int)
    if planted:
        g[bad_g] = [np.nan, np.inf, -np.inf, np.nan, np.nan]
        m[ovf], v[ovf], g[ovf] = F(3e38), F(0), F(1)
    gp, gm, gv, flag = ops.adam(p, g, m, v, hp["lr"], hp["wd"], hp["b1"], hp["b2"], hp["cb1"], hp["cb2"], hp["eps"])
    assert flag == (1 if planted else 0)
    keep = np.zeros(n, bool)
    keep[ovf] = True
    assert np.array_equal(gp[ovf], p[ovf]), "an overflowing update must keep p"
    for i in range(0, n, 1 << 22):  # the float64 reference in blocks (host memory)
        sl = slice(i, i + (1 << 22))
        (rp, Ap), (rm, Am), (rv, Av) = E.adam_ref(p[sl], g[sl], m[sl], v[sl], **hp)
        ok = ~keep[sl]
        for name, got, ref, A, sel in (("p", gp[sl], rp, Ap, ok), ("m", gm[sl], rm, Am, slice(None)), ("v", gv[sl], rv, Av, slice(None))):
            w, bad = R.dist_f32(got[sel], ref[sel], A[sel])
            assert bad == 0, "Adam %s: %d out of bounds in [%d, %d) (worst %.3g)" % (name, bad, i, i + (1 << 22), w)
            _record(("adam t=%d" % t, name), w)
    assert np.array_equal(gm[bad_g], m[bad_g]) and np.array_equal(gv[bad_g], v[bad_g]), "a NaN / Inf gradient must keep m and v"
    assert np.all(np.isfinite(gp)), "p must stay finite"


def test_nhwc_to_nchw_at_batch_256(ops):
    im = synth.uniform(90, N * 224 * 224 * 3, -124.0, 152.0).reshape(N, 224, 224, 3)
    got = ops.nhwc_to_nchw(im)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(im.transpose(0, 3, 1, 2)).view(np.uint32))
